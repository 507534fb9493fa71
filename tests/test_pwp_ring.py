"""The piecewise-polynomial leaf (mx_pwp_cross): R.pwp_cross / R.pwp against Python integers mod
2^64 / 2^128 at the size and value edges, in place on slot views, as a 3-out-of-3 sharing,
against the torch composition and, at degree 1, against R.pwl_cross; the gfx950 kernel bitwise
equal to the CPU twin."""
import numpy as np
import pytest
import torch

from moose_amd.ops import ring as R

SIZES = (1, 2, 3, 255, 257)  # odd: no two-u64 lanes; 257 crosses a block
KS = (1, 2, R.PWP_MAX)
DEGREES = (1, 2, 3)


def _rand(rng, shape, bits):
    n = int(np.prod(shape))
    vals = [int.from_bytes(rng.bytes(bits // 8), "little") for _ in range(n)]
    return np.array(vals, dtype=object).reshape(shape)


def _tables(rng, k, d, bits):
    """(D, CK) with top-bit-set (negative), small and random entries."""
    top = 1 << (bits - 1)
    D = [[int(v) for v in _rand(rng, (k,), bits)] for _ in range(d + 1)]
    D[1][0] = top | 5
    D[0][-1] = (1 << bits) - 3  # -3
    D[d][-1] = 2
    CK = [int(v) for v in _rand(rng, (d,), bits)]
    CK[0] = (1 << bits) - 7  # -7
    return D, CK


def _model(s0, s1, p0, p1, D, CK, bits):
    """The leaf in Python integers; planes [k, n], powers d x [n]."""
    M = (1 << bits) - 1
    k, n = s0.shape
    out = []
    for e in range(n):
        v = sum(D[0][j] * int(s0[j, e]) for j in range(k))
        for i in range(1, len(D)):
            g0 = sum(D[i][j] * int(s0[j, e]) for j in range(k))
            a0 = int(p0[i - 1][e])
            if s1 is None:
                v += (g0 + CK[i - 1]) * a0
            else:
                g1 = sum(D[i][j] * int(s1[j, e]) for j in range(k))
                v += g0 * (a0 + int(p1[i - 1][e])) + g1 * a0 + CK[i - 1] * a0
        out.append(v & M)
    return np.array(out, dtype=object)


def _cases(bits):
    rng = np.random.default_rng(bits)
    for n in SIZES:
        for k in KS:
            for d in DEGREES:
                s0, s1 = _rand(rng, (k, n), bits), _rand(rng, (k, n), bits)
                p0, p1 = _rand(rng, (d, n), bits), _rand(rng, (d, n), bits)
                # operands 2^bits - 1 and zero among the arbitrary ring values
                p0[0, 0] = s0[0, 0] = p0[d - 1, -1] = (1 << bits) - 1
                p1[-1, -1] = s1[-1, -1] = (1 << bits) - 1
                if n > 2:
                    p0[0, 1] = 0
                    s0[-1, 2] = 0
                yield n, k, d, s0, s1, p0, p1, _tables(rng, k, d, bits)


def _check_leaf(device, bits):
    for n, k, d, s0, s1, p0, p1, (D, CK) in _cases(bits):
        t = lambda a: R.from_ints(a, bits, device)  # noqa: E731
        ts = lambda a: [t(r) for r in a]  # noqa: E731
        got = R.to_ints(R.pwp_cross(t(s0), t(s1), ts(p0), ts(p1), D, CK))
        want = _model(s0, s1, p0, p1, D, CK, bits)
        assert (got == want).all(), (device, bits, n, k, d)
        plain = R.to_ints(R.pwp(t(s0), ts(p0), D, CK))
        assert (plain == _model(s0, None, p0, None, D, CK, bits)).all(), (bits, n, k, d)
        same = R.to_ints(R.pwp_cross(t(s0), t(np.zeros_like(s1)), ts(p0), ts(np.zeros_like(p1)),
                                     D, CK))
        assert (plain == same).all()  # plain mode = cross mode with zero next components
        tor = R.to_ints(R.pwp_torch(t(s0), t(s1), ts(p0), ts(p1), D, CK))
        assert (tor == want).all(), ("torch", device, bits, n, k, d)
        if d == 1:
            pwl = R.pwl_cross(t(s0), t(s1), t(p0[0]), t(p1[0]), D[1], D[0], CK[0])
            assert (R.to_ints(pwl) == got).all(), ("pwl", device, bits, n, k)


@pytest.mark.parametrize("bits", [64, 128])
def test_leaf_matches_python_integers_cpu(bits):
    _check_leaf("cpu", bits)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [64, 128])
def test_leaf_matches_python_integers_gpu(bits):
    _check_leaf("cuda:0", bits)


def _pair_views(buf, bits):
    """s0 = buf[0:3], s1 = buf[1:4] of a four-slot buffer (the stacked session's share pair)."""
    return R.RT(buf.data[0:3], bits), R.RT(buf.data[1:4], bits)


def _check_views(device, bits):
    rng = np.random.default_rng(7 + bits)
    for n, k, d in ((6, 2, 3), (255, 3, 2), (258, R.PWP_MAX, 3)):
        D, CK = _tables(rng, k, d, bits)
        sbuf = R.from_ints(_rand(rng, (4, k, n), bits), bits, device)
        pbufs = [R.from_ints(_rand(rng, (4, n), bits), bits, device) for _ in range(d)]
        s0, s1 = _pair_views(sbuf, bits)
        pairs = [_pair_views(b, bits) for b in pbufs]  # each power in a buffer of its own
        p0, p1 = [a for a, _ in pairs], [b for _, b in pairs]
        assert p0[0].data.untyped_storage().data_ptr() == p1[0].data.untyped_storage().data_ptr()
        got = R.pwp_cross(s0, s1, p0, p1, D, CK, nb=1)
        dense = R.pwp_cross(s0.clone(), s1.clone(), [a.clone() for a in p0],
                            [a.clone() for a in p1], D, CK, nb=1)
        assert torch.equal(got.data, dense.data)
        si, pi = R.to_ints(sbuf), [R.to_ints(b) for b in pbufs]
        for p in range(3):
            want = _model(si[p], si[p + 1], [a[p] for a in pi], [a[p + 1] for a in pi], D, CK,
                          bits)
            assert (R.to_ints(got)[p] == want).all(), (device, bits, n, k, d, p)
        # a slot stride larger than the slot: every other slot of a wider buffer
        wide_s = R.from_ints(_rand(rng, (6, k, n), bits), bits, device)
        wide_p = [R.from_ints(_rand(rng, (6, n), bits), bits, device) for _ in range(d)]
        vs, vp = R.RT(wide_s.data[::2], bits), [R.RT(w.data[::2], bits) for w in wide_p]
        got = R.pwp(vs, vp, D, CK, nb=1)
        assert torch.equal(got.data, R.pwp(vs.contiguous(), [a.contiguous() for a in vp], D, CK,
                                           nb=1).data)
        wi, wp = R.to_ints(wide_s), [R.to_ints(w) for w in wide_p]
        for p in range(3):
            assert (R.to_ints(got)[p] == _model(wi[2 * p], None, [a[2 * p] for a in wp], None, D,
                                                CK, bits)).all()


@pytest.mark.parametrize("bits", [64, 128])
def test_slot_views_are_read_in_place_cpu(bits):
    _check_views("cpu", bits)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [64, 128])
def test_slot_views_are_read_in_place_gpu(bits):
    _check_views("cuda:0", bits)


def _check_sharing(device, bits):
    """The three parties' outputs sum to sum_i (CK_i + G_i) * P_i + H of the reconstructed
    flags and powers, for random replicated sharings."""
    rng = np.random.default_rng(11 + bits)
    M = (1 << bits) - 1
    n, k = 37, 3
    for d in DEGREES:
        D, CK = _tables(rng, k, d, bits)
        sv, pv = _rand(rng, (3, k, n), bits), _rand(rng, (d, 3, n), bits)
        s0 = R.from_ints(sv, bits, device)
        p0 = [R.from_ints(pv[i], bits, device) for i in range(d)]
        s1 = R.RT(torch.roll(s0.data, -1, dims=0), bits)
        p1 = [R.RT(torch.roll(a.data, -1, dims=0), bits) for a in p0]
        v = R.to_ints(R.pwp_cross(s0, s1, p0, p1, D, CK, nb=1))
        total = (v[0] + v[1] + v[2]) & M
        s = (sv[0] + sv[1] + sv[2]) & M
        P = [(pv[i][0] + pv[i][1] + pv[i][2]) & M for i in range(d)]
        for e in range(n):
            want = sum(D[0][j] * int(s[j, e]) for j in range(k))
            for i in range(1, d + 1):
                g = sum(D[i][j] * int(s[j, e]) for j in range(k))
                want += (CK[i - 1] + g) * int(P[i - 1][e])
            assert int(total[e]) == want & M, (device, bits, d, e)


@pytest.mark.parametrize("bits", [64, 128])
def test_parties_sum_to_the_function_cpu(bits):
    _check_sharing("cpu", bits)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [64, 128])
def test_parties_sum_to_the_function_gpu(bits):
    _check_sharing("cuda:0", bits)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [64, 128])
def test_kernel_is_bitwise_the_cpu_twin(bits):
    """Dense slots at an even, a block-crossing odd (no two-u64 lanes) and a tiny odd n, and
    one call whose share pairs are the non-contiguous [0:3] / [1:4] views of four-slot
    buffers."""
    rng = np.random.default_rng(3 + bits)
    for n, k, d, views in ((257, 2, 3, False), (1024, R.PWP_MAX, 3, False), (3, 1, 1, False),
                           (514, R.PWP_MAX, 2, True), (255, 3, 3, True)):
        D, CK = _tables(rng, k, d, bits)
        if views:
            sbuf = R.from_ints(_rand(rng, (4, k, n), bits), bits)
            pbufs = [R.from_ints(_rand(rng, (4, n), bits), bits) for _ in range(d)]
            pick = lambda b, dev: _pair_views(R.RT(b.data.to(dev), bits), bits)  # noqa: E731
        else:
            sbuf = (R.from_ints(_rand(rng, (3, k, n), bits), bits),
                    R.from_ints(_rand(rng, (3, k, n), bits), bits))
            pbufs = [(R.from_ints(_rand(rng, (3, n), bits), bits),
                      R.from_ints(_rand(rng, (3, n), bits), bits)) for _ in range(d)]
            pick = lambda b, dev: tuple(R.RT(t.data.to(dev), bits) for t in b)  # noqa: E731

        def run(dev):
            s0, s1 = pick(sbuf, dev)
            pairs = [pick(b, dev) for b in pbufs]
            return R.pwp_cross(s0, s1, [a for a, _ in pairs], [b for _, b in pairs], D, CK, nb=1)

        cpu = run("cpu")
        for flag in (True, False):  # the kernel, and the composition it can be switched to
            old, R.PWP_KERNEL = R.PWP_KERNEL, flag
            try:
                got = run("cuda:0")
            finally:
                R.PWP_KERNEL = old
            assert torch.equal(got.data.cpu(), cpu.data), (bits, n, k, d, views, flag)


def test_bad_operands_are_rejected():
    z = lambda *shape, bits=64: R.zeros(shape, bits, "cpu")  # noqa: E731
    s, x = z(2, 4), z(4)
    with pytest.raises(ValueError, match="flag planes"):  # k = 0
        R.pwp(z(0, 4), [x], [[], []], [0])
    big = R.PWP_MAX + 1
    with pytest.raises(ValueError, match="flag planes"):  # k = 9
        R.pwp(z(big, 4), [x], [[1] * big, [0] * big], [0])
    with pytest.raises(ValueError, match="degree between 1 and 3"):  # d = 4
        R.pwp(s, [x] * 4, [[1, 2]] * 5, [0] * 4)
    with pytest.raises(ValueError, match="degree between 1 and 3"):  # d = 0
        R.pwp(s, [], [[1, 2]], [])
    with pytest.raises(ValueError, match="flag planes"):  # rows of different lengths
        R.pwp(s, [x, x], [[1, 2], [1, 2], [1]], [0, 0])
    with pytest.raises(ValueError, match="last-piece coefficients"):
        R.pwp(s, [x, x], [[1, 2]] * 3, [0])
    with pytest.raises(ValueError, match="2 powers per component"):
        R.pwp(s, [x], [[1, 2]] * 3, [0, 0])
    with pytest.raises(ValueError, match="expected"):
        R.pwp(s, [x, z(5)], [[1, 2]] * 3, [0, 0])
    with pytest.raises(ValueError, match="both next components"):
        R.pwp_cross(s, s, [x], None, [[1, 2]] * 2, [0])
    with pytest.raises(ValueError, match="arithmetic only"):  # mixed rings
        R.pwp(s, [z(4, bits=128)], [[1, 2]] * 2, [0])
    with pytest.raises(ValueError, match="arithmetic only"):  # bit tensors
        R.pwp(z(2, 4, bits=1), [z(4, bits=1)], [[1, 0]] * 2, [1])


def test_a_slot_stride_whose_extent_would_wrap_is_refused():
    """mx_pwp_cross bounds n * k and every slot stride -- the flags' and each power's -- by
    2^61 / slots before any (slots - 1) * stride is formed: -3, nothing read."""
    import ctypes

    from moose_amd.ops import native as nat

    bufs = [torch.zeros(64, dtype=torch.int64) for _ in range(4)]
    tab = torch.zeros(32, dtype=torch.int64)

    def call(slots, sst, pst, n=4, k=2, d=2):
        ptrs = (ctypes.c_void_p * d)(*[nat.ptr(bufs[1])] * d)
        return nat.lib().mx_pwp_cross(0, 8, nat.ptr(bufs[0]), None, ptrs, None, nat.ptr(bufs[3]),
                                      slots, sst, (ctypes.c_int64 * d)(*pst), n, k, d,
                                      nat.ptr(tab), nat.ptr(tab), None)

    assert call(1, 8, (4, 4)) == 0
    for slots, far in ((4, 1 << 61), (3, (1 << 62) + 1)):
        assert call(slots, far, (4, 4)) == -3
        assert call(slots, 8, (far, 4)) == -3
        assert call(slots, 8, (4, far)) == -3
    assert call(4, 8, (4, 4), n=1 << 59) == -3  # k * n of a slot
    assert call(1 << 40, 8, (4, 4), n=1 << 22) == -3  # slots * n
