"""The compare-exchange leaves (mx_cswap_diff / _cross / _apply): R.cswap_diff, R.cswap_cross and
R.cswap_apply against Python integers mod 2^64 / 2^128 over every stage of small networks, both
directions and the table mode, in place on slot views, against the torch compositions, and as a
whole network run in the clear; the gfx950 kernels bitwise equal to the CPU twins."""
import functools

import numpy as np
import pytest
import torch

from moose_amd.ops import ring as R

# (outer, n, inner): one pair; a block of two; columns; 260 pairs (crosses a 256-thread block,
# odd rows); a long axis; odd inner with several rows
SHAPES = ((1, 2, 1), (3, 4, 1), (1, 8, 3), (65, 8, 1), (1, 1024, 1), (2, 16, 5))


def _rand(rng, shape, bits):
    n = int(np.prod(shape))
    vals = [int.from_bytes(rng.bytes(bits // 8), "little") for _ in range(n)]
    return np.array(vals, dtype=object).reshape(shape)


def _pairs(n, k, j, desc):
    """(t, i, l, ascending) as the issue words it: i is t with a zero bit inserted at log2 j."""
    lj = j.bit_length() - 1
    for t in range(n // 2):
        i = ((t >> lj) << (lj + 1)) | (t & (j - 1))
        yield t, i, i | j, ((i & k) == 0) != desc


def _model(g, bits, x0, x1=None, s0=None, s1=None, p=None):
    """The three leaves in Python integers on [outer, n, inner] arrays: (diff, cross, apply)."""
    M = (1 << bits) - 1
    cols = range(g.inner) if g.by < 0 else [g.by]
    diff = np.zeros((g.outer, g.n // 2, len(cols)), dtype=object)
    cross = np.zeros((g.outer, g.n // 2, g.inner), dtype=object)
    out = x0.copy()
    for o in range(g.outer):
        for t, i, l, asc in _pairs(g.n, g.k, g.j, bool(g.descending)):
            for cc, c in enumerate(cols):
                diff[o, t, cc] = (x0[o, l, c] - x0[o, i, c] if asc else x0[o, i, c] - x0[o, l, c]) & M
            for c in range(g.inner):
                if s0 is not None:
                    f = 0 if g.by >= 0 else c
                    d0 = x0[o, i, c] - x0[o, l, c]
                    v = s0[o, t, f] * d0 if x1 is None else \
                        s0[o, t, f] * (d0 + x1[o, i, c] - x1[o, l, c]) + s1[o, t, f] * d0
                    cross[o, t, c] = v & M
                if p is not None:
                    out[o, i, c] = (x0[o, i, c] - p[o, t, c]) & M
                    out[o, l, c] = (x0[o, l, c] + p[o, t, c]) & M
    return diff, cross, out


def _stages(n):
    """Every j from 1 to n/2 with k in {2j, n}, both directions."""
    j = 1
    while j <= n // 2:
        for k in sorted({2 * j, n}):
            for desc in (False, True):
                yield k, j, desc
        j *= 2


@functools.lru_cache(maxsize=None)
def _cases(bits):
    """(geometry, inputs, model results), computed once and shared by the CPU and GPU tests."""
    rng = np.random.default_rng(bits)
    top = (1 << bits) - 1
    out = []
    for outer, n, inner in SHAPES:
        x0, x1 = _rand(rng, (outer, n, inner), bits), _rand(rng, (outer, n, inner), bits)
        p = _rand(rng, (outer, n // 2, inner), bits)
        # 2^bits - 1 and zero among the arbitrary ring values
        x0[0, 0, 0], x0[0, 1, 0], x1[-1, -1, -1], p[0, 0, 0] = top, 0, top, top
        for by in sorted({-1, 0, inner - 1}):
            cols = inner if by < 0 else 1
            s0, s1 = _rand(rng, (outer, n // 2, cols), bits), _rand(rng, (outer, n // 2, cols), bits)
            s0[0, 0, 0], s1[-1, -1, -1] = top, 0
            for k, j, desc in _stages(n):
                g = R.CswapGeom(outer, n, inner, by, k, j, desc)
                want = _model(g, bits, x0, x1, s0, s1, p)
                plain = _model(g, bits, x0, None, s0, None, None)[1]
                out.append((g, x0, x1, s0, s1, p, want, plain))
    return out


def _leaves(g, t, x0, x1, s0, s1, p):
    return (R.cswap_diff(t(x0), g), R.cswap_cross(t(s0), t(s1), t(x0), t(x1), g),
            R.cswap_apply(t(x0), t(p), g), R.cswap_cross(t(s0), None, t(x0), None, g))


def _check_leaf_cpu(bits):
    t = lambda a: R.from_ints(a, bits, "cpu")  # noqa: E731
    for g, x0, x1, s0, s1, p, want, plain in _cases(bits):
        d, c, a, pl = _leaves(g, t, x0, x1, s0, s1, p)
        assert tuple(d.shape) == want[0].shape and tuple(a.shape) == x0.shape
        assert (R.to_ints(d) == want[0]).all(), ("diff", bits, g)
        assert (R.to_ints(c) == want[1]).all(), ("cross", bits, g)
        assert (R.to_ints(a) == want[2]).all(), ("apply", bits, g)
        assert (R.to_ints(pl) == plain).all(), ("plain", bits, g)
        zero = t(np.zeros_like(s1)), t(np.zeros_like(x1))
        same = R.cswap_cross(t(s0), zero[0], t(x0), zero[1], g)
        assert torch.equal(same.data, pl.data)  # plain mode = cross mode with zero next components
        assert (R.to_ints(R.cswap_diff_torch(t(x0), g)) == want[0]).all(), ("torch diff", g)
        assert (R.to_ints(R.cswap_cross_torch(t(s0), t(s1), t(x0), t(x1), g)) == want[1]).all(), g
        assert (R.to_ints(R.cswap_cross_torch(t(s0), None, t(x0), None, g)) == plain).all(), g
        assert (R.to_ints(R.cswap_apply_torch(t(x0), t(p), g)) == want[2]).all(), ("torch", g)


@pytest.mark.parametrize("bits", [64, 128])
def test_leaves_match_python_integers_cpu(bits):
    _check_leaf_cpu(bits)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [64, 128])
def test_leaves_gpu_equal_cpu_bitwise(bits):
    tc = lambda a: R.from_ints(a, bits, "cpu")  # noqa: E731
    uploaded = {}

    def tg(a):  # one upload per array
        if id(a) not in uploaded:
            uploaded[id(a)] = R.from_ints(a, bits, "cuda:0")
        return uploaded[id(a)]

    for g, x0, x1, s0, s1, p, _want, _plain in _cases(bits):
        cpu = _leaves(g, tc, x0, x1, s0, s1, p)
        gpu = _leaves(g, tg, x0, x1, s0, s1, p)
        tor = (R.cswap_diff_torch(tg(x0), g), R.cswap_cross_torch(tg(s0), tg(s1), tg(x0), tg(x1), g),
               R.cswap_apply_torch(tg(x0), tg(p), g))
        for name, a, b in zip(("diff", "cross", "apply", "plain"), cpu, gpu):
            assert torch.equal(a.data, b.data.cpu()), (name, bits, g)
        for name, a, b in zip(("diff", "cross", "apply"), cpu, tor):
            assert torch.equal(a.data, b.data.cpu()), ("torch " + name, bits, g)


def _pair_views(buf, bits):
    """s0 = buf[0:3], s1 = buf[1:4] of a four-slot buffer (the stacked session's share pair)."""
    return R.RT(buf.data[0:3], bits), R.RT(buf.data[1:4], bits)


def _check_views(device, bits):
    rng = np.random.default_rng(11 + bits)
    for (outer, n, inner), by, k, j, desc in (((3, 4, 1), -1, 2, 1, False), ((1, 8, 3), 2, 8, 2, True),
                                              ((65, 8, 1), -1, 8, 4, False),
                                              ((2, 16, 5), 0, 16, 1, True)):
        g = R.CswapGeom(outer, n, inner, by, k, j, desc)
        cols = g.cols
        xi, si = _rand(rng, (4, outer, n, inner), bits), _rand(rng, (4, outer, n // 2, cols), bits)
        pi = _rand(rng, (4, outer, n // 2, inner), bits)
        xbuf, sbuf, pbuf = (R.from_ints(a, bits, device) for a in (xi, si, pi))
        x0, x1 = _pair_views(xbuf, bits)
        s0, s1 = _pair_views(sbuf, bits)
        assert x0.data.untyped_storage().data_ptr() == x1.data.untyped_storage().data_ptr()
        cross = R.cswap_cross(s0, s1, x0, x1, g, nb=1)
        assert torch.equal(cross.data, R.cswap_cross(s0.clone(), s1.clone(), x0.clone(),
                                                     x1.clone(), g, nb=1).data)
        # the share-wise leaves over all four slots in one launch, and on each view
        diff4, app4 = R.cswap_diff(xbuf, g, nb=1), R.cswap_apply(xbuf, pbuf, g, nb=1)
        p0, p1 = _pair_views(pbuf, bits)
        for lo, xv, pv in ((0, x0, p0), (1, x1, p1)):
            assert torch.equal(R.cswap_diff(xv, g, nb=1).data, diff4.data[lo:lo + 3])
            assert torch.equal(R.cswap_apply(xv, pv, g, nb=1).data, app4.data[lo:lo + 3])
        dg, cg, ag = R.to_ints(diff4), R.to_ints(cross), R.to_ints(app4)
        for q in range(4):
            nxt = min(q + 1, 3)
            want = _model(g, bits, xi[q], xi[nxt], si[q], si[nxt], pi[q])
            assert (dg[q] == want[0]).all() and (ag[q] == want[2]).all(), (device, bits, g, q)
            if q < 3:
                assert (cg[q] == want[1]).all(), (device, bits, g, q)
        # a slot stride larger than the slot: every other slot of a wider buffer
        wide = R.from_ints(_rand(rng, (6, outer, n, inner), bits), bits, device)
        v = R.RT(wide.data[::2], bits)
        assert torch.equal(R.cswap_diff(v, g, nb=1).data, R.cswap_diff(v.contiguous(), g, nb=1).data)


@pytest.mark.parametrize("bits", [64, 128])
def test_slot_views_in_place_cpu(bits):
    _check_views("cpu", bits)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [64, 128])
def test_slot_views_in_place_gpu(bits):
    _check_views("cuda:0", bits)


def _network_in_the_clear(device, bits, outer, n, inner, by, desc, rng):
    """diff -> the true sign -> plain cross -> apply over every stage, on ordinary integers."""
    vals = rng.integers(-1000, 1000, size=(outer, n, inner))
    if by >= 0:  # distinct keys: the order of the rows is determined
        for o in range(outer):
            vals[o, :, by] = rng.permutation(n) - n // 2
    x = R.from_ints(np.vectorize(lambda v: int(v) % (1 << bits), otypes=[object])(vals), bits, device)
    stages = R.cswap_stages(n)
    assert len(stages) == (n.bit_length() - 1) * n.bit_length() // 2
    for k, j in stages:
        g = R.CswapGeom(outer, n, inner, by, k, j, desc)
        c = R.to_signed_ints(R.cswap_diff(x, g))
        s = R.from_ints(np.vectorize(lambda v: int(v < 0), otypes=[object])(c), bits, device)
        x = R.cswap_apply(x, R.cswap_cross(s, None, x, None, g), g)
    got = R.to_signed_ints(x).astype(np.int64)
    if by < 0:
        want = np.sort(vals, axis=1)
        want = want[:, ::-1] if desc else want
    else:
        order = np.argsort(vals[:, :, by], axis=1)
        order = order[:, ::-1] if desc else order
        want = np.take_along_axis(vals, order[:, :, None], axis=1)
    assert (got == want).all(), (device, bits, outer, n, inner, by, desc)


def _check_network(device):
    rng = np.random.default_rng(5)
    for bits in (64, 128):
        for n in (2, 8, 64):
            for desc in (False, True):
                _network_in_the_clear(device, bits, 2, n, 1, -1, desc, rng)
        _network_in_the_clear(device, bits, 1, 8, 3, -1, False, rng)
        _network_in_the_clear(device, bits, 2, 8, 3, 1, True, rng)


def test_network_in_the_clear_sorts_cpu():
    _check_network("cpu")


@pytest.mark.gpu
def test_network_in_the_clear_sorts_gpu():
    _check_network("cuda:0")


def test_malformed_stage_is_refused():
    x = R.from_ints(np.arange(8, dtype=object), 64, "cpu")
    for bad in (R.CswapGeom(1, 6, 1, -1, 2, 1), R.CswapGeom(1, 8, 1, -1, 2, 2),
                R.CswapGeom(1, 8, 1, -1, 16, 1), R.CswapGeom(1, 8, 1, 1, 2, 1),
                R.CswapGeom(2, 8, 1, -1, 2, 1)):
        with pytest.raises(ValueError):
            R.cswap_diff(x, bad)


def test_a_slot_stride_whose_extent_would_wrap_is_refused():
    """The three mx_cswap_* entries bound n_x and every slot stride by 2^61 / slots before any
    (slots - 1) * stride is formed: -3, nothing read."""
    from moose_amd.ops import native as nat

    bufs = [torch.zeros(64, dtype=torch.int64) for _ in range(4)]
    p = [nat.ptr(b) for b in bufs]
    geom = (1, 8, 1, -1, 2, 1, 0)  # outer, n, inner, by, k, j, descending
    L = nat.lib()

    def diff(slots, xst, g=geom):
        return L.mx_cswap_diff(0, 8, p[0], p[3], slots, xst, *g, None)

    def cross(slots, sst, xst):
        return L.mx_cswap_cross(0, 8, p[1], None, p[0], None, p[3], slots, sst, xst, *geom, None)

    def apply(slots, xst, pst):
        return L.mx_cswap_apply(0, 8, p[0], p[1], p[3], slots, xst, pst, *geom, None)

    assert diff(1, 8) == 0 and cross(1, 4, 8) == 0 and apply(1, 8, 4) == 0
    for slots, far in ((4, 1 << 61), (3, (1 << 62) + 1)):
        assert diff(slots, far) == -3
        assert cross(slots, far, 8) == -3 and cross(slots, 4, far) == -3
        assert apply(slots, far, 4) == -3 and apply(slots, 8, far) == -3
    assert diff(4, 8, (1 << 30, 1 << 30, 1, -1, 2, 1, 0)) == -3  # slots * n_x = 2^62
