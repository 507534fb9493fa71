"""The share-source CRT prep (k_crt_prep_src) takes the image of a sum of two share slots
from the two slots' residues instead of a third full residue pass: with S(.) the signed
representative, S(r + v mod 2^128) = S(r) + S(v) + kappa 2^128 with kappa = top(r) + top(v) -
carry - top(r + v) in {-1, 0, 1}, and 2^128 = -neg (mod p), so the sum's residue is the
centred residue of ra + rb - kappa neg.

CPU: that combine (mx_crt_combine: the function the kernel calls) against python integers,
over every modulus, every kappa and every pair of centred residues, and on 128-bit pairs
with the edge values.  GPU: the product from share sources stays bitwise mx_share3_k +
mx_gemm_asym on uniformly random 128-bit ring data, where a quarter of the elements take a
correction (fixed-point sized inputs would never run it), and on the placements that emit a
phase twice, no sum, or the zero phase."""
import numpy as np
import pytest
import torch

from moose_amd.ir.computation import ReplicatedPlacement
from moose_amd.ops import native as nat
from moose_amd.ops import ring as R
from moose_amd.runtime.session import StackedSession

PLC = ReplicatedPlacement(("alice", "bob", "carole"))
N_MOD = 36  # Z_2^128 at the largest inner dimension of one call
MASK = (1 << 128) - 1
NX, NY = 0x51, 0x1_0000_0007
RING = 0  # kind code: ring data (MX_CROSS_ARITH)


def _ptr(a):
    return a.ctypes.data_as(nat.ctypes.c_void_p)


def _tables():
    """p, the byte weights of the A (inverse folded in) and B residues, and neg = -2^128
    (times the folded inverse) mod p.  mx_crt_tables reports p = 256's multiplier in neg's
    place; 2^128 mod 256 is 0."""
    n = N_MOD
    p = np.zeros(n, np.int32)
    wa, wb = np.zeros((n, 16), np.uint8), np.zeros((n, 16), np.uint8)
    nega, negb = np.zeros(n, np.int32), np.zeros(n, np.int32)
    W, Mw = np.zeros((n, 8), np.uint16), np.zeros(8, np.uint16)
    assert nat.lib().mx_crt_tables(2, n, _ptr(p), _ptr(wa), _ptr(wb), _ptr(nega), _ptr(negb),
                                   _ptr(W), _ptr(Mw)) == 0
    mul0 = {"a": int(nega[0]), "b": int(negb[0])}
    nega[0] = negb[0] = 0
    return dict(p=[int(v) for v in p], w={"a": wa.astype(np.int64), "b": wb.astype(np.int64)},
                neg={"a": nega.astype(np.int64), "b": negb.astype(np.int64)}, mul0=mul0)


def _centered(s, p):
    return (s + p // 2) % p - p // 2


def _combine(side, i, ra, rb, kappa):
    """The bytes the kernel stores for modulus i (side a: the packed form, b: the scalar)."""
    ra, rb, kappa = (np.ascontiguousarray(v, np.int32) for v in (ra, rb, kappa))
    out = np.zeros(len(ra), np.int8)
    assert nat.lib().mx_crt_combine(2, N_MOD, "ab".index(side), i, len(ra), _ptr(ra), _ptr(rb),
                                    _ptr(kappa), _ptr(out)) == 0
    return out.astype(np.int64)


@pytest.mark.parametrize("side", ["a", "b"])
def test_combine_every_residue_pair(side):
    """Every modulus, kappa in {-1, 0, 1}, every pair of centred residues (p^2 of them)."""
    t = _tables()
    for i, p in enumerate(t["p"]):
        neg = int(t["neg"][side][i])
        res = np.arange(-(p // 2), p - p // 2, dtype=np.int64)  # p odd: +-(p-1)/2; 256: -128..127
        assert len(res) == p
        ra, rb, kappa = (v.ravel() for v in np.meshgrid(res, res, np.array([-1, 0, 1]),
                                                        indexing="ij"))
        want = _centered(ra + rb - kappa * neg, p)
        got = _combine(side, i, ra, rb, kappa)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (side, p, ra[bad[:4]], rb[bad[:4]], kappa[bad[:4]])


def _residue(x, side, i, t):
    """Centred residue of ring element x (python int) as the preps compute it."""
    p = t["p"][i]
    if i == 0:  # the low byte times the folded inverse
        return _centered((x & 0xFF) * t["mul0"][side], 256)
    s = sum(((x >> (8 * j)) & 0xFF) * int(t["w"][side][i][j]) for j in range(16))
    return _centered(s + (x >> 127) * int(t["neg"][side][i]), p)


def _edge_pairs():
    w80, wff = 0x80808080, 0xFFFFFFFF
    edge = [0, MASK, (1 << 127) - 1, 1 << 127, 1, (1 << 127) + 1, (1 << 128) - 2]
    for word in (w80, wff):  # words with every byte 0x80 / 0xff, in every subset of the four
        for m in range(1, 16):
            edge.append(sum(word << (32 * q) for q in range(4) if m >> q & 1))
    rng = np.random.default_rng(11)
    rnd = [int.from_bytes(rng.bytes(16), "little") for _ in range(600)]
    pairs = [(a, b) for a in edge for b in edge]
    pairs += [(a, b) for a in edge for b in rnd[:8]] + [(b, a) for a in edge for b in rnd[:8]]
    pairs += list(zip(rnd[0::2], rnd[1::2]))
    return pairs


@pytest.mark.parametrize("side", ["a", "b"])
def test_combine_wrapped_sums(side):
    """128-bit pairs with 0, -1, 2^127 - 1, -2^127 and all-0xff / all-0x80 words: kappa from
    the top bits and the carry; the combined residue is that of the wrapped sum."""
    t = _tables()
    pairs = _edge_pairs()
    kappa = np.array([(a >> 127) + (b >> 127) - ((a + b) >> 128) - (((a + b) & MASK) >> 127)
                      for a, b in pairs])
    assert set(kappa.tolist()) == {-1, 0, 1}
    for i, p in enumerate(t["p"]):
        ra = np.array([_residue(a, side, i, t) for a, _ in pairs])
        rb = np.array([_residue(b, side, i, t) for _, b in pairs])
        want = np.array([_residue((a + b) & MASK, side, i, t) for a, b in pairs])
        got = _combine(side, i, ra, rb, kappa)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (side, p, [pairs[k] for k in bad[:3]])


# -- GPU ---------------------------------------------------------------------------------------
def _bits_of(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def _uniform(shape, seed):
    """Uniformly random 128-bit ring data, (low, high) words."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randint(0, 256, (shape[0] * shape[1] * 16,), generator=g, dtype=torch.uint8)
    return raw.view(torch.int64).reshape(shape + (2,)).cuda()


def _issued(sess, xd, shape, j0, d, nonce):
    """The arguments of a ring-data sharing by owner j0 in direction d."""
    return (RING | (R.SHARE_MIRROR if d == 2 else 0), xd, 0, j0,
            sess.key_ptr(PLC, (j0 + d - 1) % 3), nonce, tuple(shape), 128)


def _phases(side, j0, d):
    """launch_prep_src's plan: the phase (0 = r, 1 = x - r, 2 = their sum, 3 = zero) of each
    of the side's four images, A = [x0 + x1, x2, x1, x0], B = [y0 + y1, y1 + y2, y2, y0]."""
    jr, jv = ((j0 + 1) % 3, j0) if d == 2 else (j0, (j0 + 1) % 3)
    slots = {"x": [(0, 1), (2,), (1,), (0,)], "y": [(0, 1), (1, 2), (2,), (0,)]}[side]
    return [2 if jr in s and jv in s else 0 if jr in s else 1 if jv in s else 3 for s in slots]


def _kappa_counts(stack, a, b):
    """Elements of slot a + slot b with kappa = -1, 0, +1, from the written shares."""
    w = _bits_of(stack).numpy().view(np.uint64)  # [3, R, C, 2] (low, high)
    la, ha, lb, hb = w[a, ..., 0], w[a, ..., 1], w[b, ..., 0], w[b, ..., 1]
    c = ((la + lb) < la).astype(np.uint64)
    t = ha + hb
    uh = t + c
    carry = ((t < ha) | (uh < t)).astype(np.int64)
    top = lambda h: (h >> np.uint64(63)).astype(np.int64)  # noqa: E731
    kappa = top(ha) + top(hb) - carry - top(uh)
    return [int((kappa == k).sum()) for k in (-1, 0, 1)]


class _Case:
    """One shape's operands, the share stacks mx_share3_k writes and mx_gemm_asym's products
    on them, each computed once."""

    def __init__(self, mkn):
        self.M, self.K, self.N = mkn
        self.sess = StackedSession("cuda", seed=7)
        self.x, self.y = _uniform((self.M, self.K), 1), _uniform((self.K, self.N), 2)
        self.stacks, self.want = {}, {}

    def args(self, name, j0, d):
        t, shape, nonce = ((self.x, (self.M, self.K), NX) if name == "x"
                           else (self.y, (self.K, self.N), NY))
        return _issued(self.sess, t, shape, j0, d, nonce)

    def stack(self, name, j0, d):
        key = (name, j0, d)
        if key not in self.stacks:
            s0, _ = self.sess.fused_share_run(PLC, self.args(name, j0, d))
            self.stacks[key] = s0.v
        return self.stacks[key]

    def check(self, side, j0, d):
        xo, yo = ((j0, d) if "x" in side else (1, 1)), ((j0, d) if "y" in side else (1, 1))
        if (xo, yo) not in self.want:
            self.want[xo, yo] = _bits_of(R.dot_cross_asym(self.stack("x", *xo), None,
                                                          self.stack("y", *yo), None,
                                                          rolled=True).data)
        got = R.dot_cross_asym_src(None if "x" in side else self.stack("x", 1, 1),
                                   None if "y" in side else self.stack("y", 1, 1),
                                   self.args("x", j0, d)[:6] if "x" in side else None,
                                   self.args("y", j0, d)[:6] if "y" in side else None,
                                   self.M, self.K, self.N)
        assert got is not None, (side, j0, d)
        assert tuple(got.shape) == (3, self.M, self.N)
        assert torch.equal(_bits_of(got.data), self.want[xo, yo]), (side, j0, d)


@pytest.mark.gpu
@pytest.mark.parametrize("mkn", [(256, 256, 256), (300, 512, 256)])
def test_uniform_ring_data_matches_share_then_gemm(mkn):
    """One tile and one chunk group; ragged rows and two chunk groups.  x only, y only and
    both, every owner, both directions.  Every sum image's three kappa classes are populated
    (about an eighth of the elements each for +-1)."""
    case = _Case(mkn)
    for j0 in range(3):
        for d in (1, 2):
            for side in ("x", "y", "xy"):
                case.check(side, j0, d)
            for name in ("x", "y"):
                slots = {"x": [(0, 1)], "y": [(0, 1), (1, 2)]}[name]
                for e, ph in enumerate(_phases(name, j0, d)[:len(slots)]):
                    if ph == 2:
                        counts = _kappa_counts(case.stack(name, j0, d).data, *slots[e])
                        print("kappa", mkn, name, j0, d, counts)
                        assert min(counts) >= 1000, (name, j0, d, counts)
    sums = [(n, j0) for n in "xy" for j0 in range(3) if 2 in _phases(n, j0, 1)]
    assert sums == [("x", 0), ("y", 0), ("y", 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("side,j0,d,phases", [
    ("x", 1, 1, [0, 1, 0, 3]),  # no sum image, r emitted twice, the zero phase
    ("y", 2, 1, [1, 0, 0, 1]),  # no sum, both slots twice, no zero phase
    ("x", 0, 2, [2, 3, 0, 1]),  # mirrored: sum and zero phase
    ("y", 1, 2, [1, 2, 0, 3]),  # the sum in the second image
])
def test_placements(side, j0, d, phases):
    assert _phases(side, j0, d) == phases
    _Case((256, 256, 256)).check(side, j0, d)
