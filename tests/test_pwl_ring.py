"""The piecewise-linear leaf (mx_pwl_cross): R.pwl_cross / R.pwl against Python integers mod
2^64 / 2^128 at the size and value edges, in place on slot views, as a 3-out-of-3 sharing, and
against the torch composition; the gfx950 kernel bitwise equal to the CPU twin."""
import numpy as np
import pytest
import torch

from moose_amd.ops import ring as R

SIZES = (1, 2, 3, 255, 257)  # odd: no two-u64 lanes; 257 crosses a block
KS = (1, 2, R.PWL_MAX)


def _rand(rng, shape, bits):
    n = int(np.prod(shape))
    vals = [int.from_bytes(rng.bytes(bits // 8), "little") for _ in range(n)]
    return np.array(vals, dtype=object).reshape(shape)


def _tables(rng, k, bits):
    """Tables with the top bit set (negative), small and random entries."""
    top = 1 << (bits - 1)
    da = [int(v) for v in _rand(rng, (k,), bits)]
    db = [int(v) for v in _rand(rng, (k,), bits)]
    da[0] = top | 5
    db[-1] = (1 << bits) - 3  # -3
    return da, db, (1 << bits) - 7  # ak = -7


def _model(s0, s1, x0, x1, da, db, ak, bits):
    """The leaf in Python integers; planes [k, n], inputs [n]."""
    M = (1 << bits) - 1
    k, n = s0.shape
    out = []
    for e in range(n):
        g0 = sum(da[j] * int(s0[j, e]) for j in range(k))
        h = sum(db[j] * int(s0[j, e]) for j in range(k))
        a0 = int(x0[e])
        if s1 is None:
            v = g0 * a0 + ak * a0 + h
        else:
            g1 = sum(da[j] * int(s1[j, e]) for j in range(k))
            v = g0 * (a0 + int(x1[e])) + g1 * a0 + ak * a0 + h
        out.append(v & M)
    return np.array(out, dtype=object)


def _cases(bits):
    rng = np.random.default_rng(bits)
    for n in SIZES:
        for k in KS:
            s0, s1 = _rand(rng, (k, n), bits), _rand(rng, (k, n), bits)
            x0, x1 = _rand(rng, (n,), bits), _rand(rng, (n,), bits)
            # operands 2^bits - 1 and zero among the arbitrary ring values
            x0[0] = s0[0, 0] = (1 << bits) - 1
            x1[-1] = s1[-1, -1] = (1 << bits) - 1
            if n > 2:
                x0[1] = 0
            yield n, k, s0, s1, x0, x1, _tables(rng, k, bits)


def _check_leaf(device, bits):
    for n, k, s0, s1, x0, x1, (da, db, ak) in _cases(bits):
        t = lambda a: R.from_ints(a, bits, device)  # noqa: E731
        got = R.to_ints(R.pwl_cross(t(s0), t(s1), t(x0), t(x1), da, db, ak))
        want = _model(s0, s1, x0, x1, da, db, ak, bits)
        assert (got == want).all(), (device, bits, n, k)
        plain = R.to_ints(R.pwl(t(s0), t(x0), da, db, ak))
        assert (plain == _model(s0, None, x0, None, da, db, ak, bits)).all(), (bits, n, k)
        zero = np.zeros_like(s1), np.zeros_like(x1)
        same = R.to_ints(R.pwl_cross(t(s0), t(zero[0]), t(x0), t(zero[1]), da, db, ak))
        assert (plain == same).all()  # plain mode = cross mode with zero next components
        tor = R.to_ints(R.pwl_torch(t(s0), t(s1), t(x0), t(x1), da, db, ak))
        assert (tor == want).all(), ("torch", device, bits, n, k)


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
    for n, k in ((6, 2), (255, 3), (258, R.PWL_MAX)):
        da, db, ak = _tables(rng, k, bits)
        sbuf = R.from_ints(_rand(rng, (4, k, n), bits), bits, device)
        xbuf = R.from_ints(_rand(rng, (4, n), bits), bits, device)
        s0, s1 = _pair_views(sbuf, bits)
        x0, x1 = _pair_views(xbuf, bits)
        assert s0.data.untyped_storage().data_ptr() == s1.data.untyped_storage().data_ptr()
        got = R.pwl_cross(s0, s1, x0, x1, da, db, ak, nb=1)
        dense = R.pwl_cross(s0.clone(), s1.clone(), x0.clone(), x1.clone(), da, db, ak, nb=1)
        assert torch.equal(got.data, dense.data)
        si, xi = R.to_ints(sbuf), R.to_ints(xbuf)
        for p in range(3):
            want = _model(si[p], si[p + 1], xi[p], xi[p + 1], da, db, ak, bits)
            assert (R.to_ints(got)[p] == want).all(), (device, bits, n, k, p)
        # a slot stride larger than the slot: every other slot of a wider buffer
        wide_s = R.from_ints(_rand(rng, (6, k, n), bits), bits, device)
        wide_x = R.from_ints(_rand(rng, (6, n), bits), bits, device)
        vs, vx = R.RT(wide_s.data[::2], bits), R.RT(wide_x.data[::2], bits)
        got = R.pwl(vs, vx, da, db, ak, nb=1)
        assert torch.equal(got.data, R.pwl(vs.contiguous(), vx.contiguous(), da, db, ak, nb=1).data)
        wi, wx = R.to_ints(wide_s), R.to_ints(wide_x)
        for p in range(3):
            assert (R.to_ints(got)[p] == _model(wi[2 * p], None, wx[2 * p], None, da, db, ak,
                                                bits)).all()


@pytest.mark.parametrize("bits", [64, 128])
def test_slot_views_are_read_in_place_cpu(bits):
    _check_views("cpu", bits)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [64, 128])
def test_slot_views_are_read_in_place_gpu(bits):
    _check_views("cuda:0", bits)


def _check_sharing(device, bits):
    """The three parties' v sum to (A_k + G) * x + H for random replicated sharings."""
    rng = np.random.default_rng(11 + bits)
    M = (1 << bits) - 1
    n, k = 37, 3
    da, db, ak = _tables(rng, k, bits)
    sv, xv = _rand(rng, (3, k, n), bits), _rand(rng, (3, n), bits)
    s0, x0 = R.from_ints(sv, bits, device), R.from_ints(xv, bits, device)
    s1 = R.RT(torch.roll(s0.data, -1, dims=0), bits)
    x1 = R.RT(torch.roll(x0.data, -1, dims=0), bits)
    v = R.to_ints(R.pwl_cross(s0, s1, x0, x1, da, db, ak, nb=1))
    total = (v[0] + v[1] + v[2]) & M
    s = (sv[0] + sv[1] + sv[2]) & M
    x = (xv[0] + xv[1] + xv[2]) & M
    for e in range(n):
        g = sum(da[j] * int(s[j, e]) for j in range(k))
        h = sum(db[j] * int(s[j, e]) for j in range(k))
        assert int(total[e]) == ((ak + g) * int(x[e]) + h) & M


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
    rng = np.random.default_rng(3 + bits)
    for n, k in ((257, 2), (1024, R.PWL_MAX), (3, 1)):
        da, db, ak = _tables(rng, k, bits)
        ops = [R.from_ints(_rand(rng, shp, bits), bits) for shp in ((3, k, n), (3, k, n), (3, n),
                                                                    (3, n))]
        cpu = R.pwl_cross(*ops, da, db, ak, nb=1)
        dev = [R.RT(o.data.to("cuda:0"), bits) for o in ops]
        for flag in (True, False):  # the kernel, and the composition it can be switched to
            old, R.PWL_KERNEL = R.PWL_KERNEL, flag
            try:
                got = R.pwl_cross(*dev, da, db, ak, nb=1)
            finally:
                R.PWL_KERNEL = old
            assert torch.equal(got.data.cpu(), cpu.data), (bits, n, k, flag)


def test_bad_operands_are_rejected():
    s, x = R.zeros((2, 4), 64, "cpu"), R.zeros((4,), 64, "cpu")
    with pytest.raises(ValueError, match="flag planes"):
        R.pwl(R.zeros((R.PWL_MAX + 1, 4), 64, "cpu"), x, [1] * (R.PWL_MAX + 1),
              [0] * (R.PWL_MAX + 1), 0)
    with pytest.raises(ValueError, match="expected"):
        R.pwl(s, R.zeros((5,), 64, "cpu"), [1, 2], [0, 0], 0)
    with pytest.raises(ValueError, match="both next components"):
        R.pwl_cross(s, s, x, None, [1, 2], [0, 0], 0)
    with pytest.raises(ValueError, match="arithmetic only"):
        R.pwl(s, R.zeros((4,), 128, "cpu"), [1, 2], [0, 0], 0)
