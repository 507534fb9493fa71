"""The outer-product leaf (mx_outer_cross): R.outer_cross in plain and cross mode and the
torch composition against Python integers mod 2^64 / 2^128, with arbitrary ring values (the
kernel is ring-bilinear); L and H as views of one buffer read in place; the return codes of
the entry; the gfx950 kernel bitwise equal to the CPU twin, its 64-bit index forms included."""
import functools

import numpy as np
import pytest
import torch

from moose_amd.ops import native as nat
from moose_amd.ops import ring as R

# (groups, rows, A, B, n_out): one element; one pair of bits; groups and odd rows; A != B both
# ways, the second with an odd n_out (the one-element u64 form); trimmed inside a run; rows
# that cross a 256-thread block; a wider square; columns that cross a lane tile, trimmed
CASES = ((1, 1, 1, 1, 1), (1, 1, 2, 2, 4), (3, 5, 2, 2, 4), (1, 3, 4, 2, 8), (1, 3, 2, 4, 7),
         (1, 2, 4, 4, 11), (2, 65, 4, 4, 16), (1, 2, 16, 16, 256), (1, 2, 256, 4, 1000))


def _rand(rng, shape, bits):
    n = int(np.prod(shape))
    vals = [int.from_bytes(rng.bytes(bits // 8), "little") for _ in range(n)]
    return np.array(vals, dtype=object).reshape(shape)


def _model(g, bits, la, ha, lb=None, hb=None):
    """out[.., c] = L[.., c % A] * H[.., c // A] (cross: La*(Ha + Hb) + Lb*Ha) in Python
    integers, on [.., groups, rows, *] arrays."""
    M = (1 << bits) - 1
    c = np.arange(g.n_out)
    a, b = c % g.A, c // g.A
    if lb is None:
        return (la[..., a] * ha[..., b]) & M
    return (la[..., a] * (ha[..., b] + hb[..., b]) + lb[..., a] * ha[..., b]) & M


@functools.lru_cache(maxsize=None)
def _cases(bits):
    """(geometry, inputs, model results), computed once and shared by the CPU and GPU tests."""
    rng = np.random.default_rng(300 + bits)
    top = (1 << bits) - 1
    out = []
    for case in CASES:
        g = R.OuterGeom(*case)
        la, lb = (_rand(rng, (g.groups, g.rows, g.A), bits) for _ in range(2))
        ha, hb = (_rand(rng, (g.groups, g.rows, g.B), bits) for _ in range(2))
        la[0, 0, 0], ha[0, 0, 0], lb[-1, -1, -1], hb[-1, -1, -1] = top, top, 0, 0
        la[-1, -1, -1], ha[-1, -1, -1] = top, 0
        out.append((g, la, lb, ha, hb, _model(g, bits, la, ha, lb, hb), _model(g, bits, la, ha)))
    return out


@pytest.mark.parametrize("bits", [64, 128])
def test_leaf_matches_python_integers_cpu(bits):
    t = lambda v: R.from_ints(v, bits, "cpu")  # noqa: E731
    for g, la, lb, ha, hb, cross, plain in _cases(bits):
        c = R.outer_cross(t(la), t(lb), t(ha), t(hb), g)
        pl = R.outer_cross(t(la), None, t(ha), None, g)
        assert tuple(c.shape) == (g.groups, g.rows, g.n_out) and c.data.is_contiguous()
        assert (R.to_ints(c) == cross).all(), ("cross", bits, g)
        assert (R.to_ints(pl) == plain).all(), ("plain", bits, g)
        # plain mode = cross mode with zero next components
        zl, zh = t(np.zeros_like(lb)), t(np.zeros_like(hb))
        assert torch.equal(R.outer_cross(t(la), zl, t(ha), zh, g).data, pl.data)
        assert (R.to_ints(R.outer_cross_torch(t(la), t(lb), t(ha), t(hb), g)) == cross).all(), g
        assert (R.to_ints(R.outer_cross_torch(t(la), None, t(ha), None, g)) == plain).all(), g


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [64, 128])
def test_leaf_gpu_equals_cpu_bitwise(bits):
    tc = lambda v: R.from_ints(v, bits, "cpu")  # noqa: E731
    tg = lambda v: R.from_ints(v, bits, "cuda:0")  # noqa: E731
    for g, la, lb, ha, hb, _cross, _plain in _cases(bits):
        cpu = (R.outer_cross(tc(la), tc(lb), tc(ha), tc(hb), g),
               R.outer_cross(tc(la), None, tc(ha), None, g))
        dl, db, dh, dd = tg(la), tg(lb), tg(ha), tg(hb)
        gpu = (R.outer_cross(dl, db, dh, dd, g), R.outer_cross(dl, None, dh, None, g))
        tor = (R.outer_cross_torch(dl, db, dh, dd, g), R.outer_cross_torch(dl, None, dh, None, g))
        for name, x, y, z in zip(("cross", "plain"), cpu, gpu, tor):
            assert torch.equal(x.data, y.data.cpu()), (name, bits, g)
            assert torch.equal(x.data, z.data.cpu()), ("torch " + name, bits, g)


class _Spy:
    """nat.lib() with every call recorded as (name, arguments)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.calls.append((name, list(args)))
            return fn(*args)

        return call


def _spied(monkeypatch, fn):
    spy = _Spy(nat.lib())
    with monkeypatch.context() as m:
        m.setattr(nat, "lib", lambda: spy)
        out = fn()
    return out, spy.calls


def _check_views(device, bits, monkeypatch):
    """A level reads the groups (2g, 2g + 1) of the previous level's output where they are: on
    the slot views of a four-slot share-pair buffer [4, G, rows, A], H = L + rows * A at a
    group stride of 2 * rows * A and the pair buffer's slot stride."""
    rng = np.random.default_rng(31 + bits)
    w = bits // 64
    for G, rows, A, n_out in ((2, 3, 2, 4), (5, 5, 2, 4), (4, 65, 4, 16), (3, 2, 16, 200)):
        g = R.OuterGeom(G // 2, rows, A, A, n_out)
        xi = _rand(rng, (4, G, rows, A), bits)
        buf = R.from_ints(xi, bits, device)
        x0, x1 = R.RT(buf.data[0:3], bits), R.RT(buf.data[1:4], bits)
        (l0, h0), (l1, h1) = R.outer_pairs(x0, nb=1), R.outer_pairs(x1, nb=1)
        assert l0.data.untyped_storage().data_ptr() == h1.data.untyped_storage().data_ptr()
        assert h0.data.data_ptr() == l0.data.data_ptr() + rows * A * 8 * w
        got, calls = _spied(monkeypatch, lambda: R.outer_cross(l0, l1, h0, h1, g, nb=1))  # noqa: B023
        assert [c[0] for c in calls] == ["mx_outer_cross"]  # one launch, no dense copy before it
        args = calls[0][1]
        # (dev, elem_bytes, la lb ha hb out, slots, l_slot l_group h_slot h_group, geometry..)
        assert args[2:6] == [l0.data.data_ptr(), l1.data.data_ptr(), h0.data.data_ptr(),
                             h1.data.data_ptr()]
        assert args[7] == 3
        group = 2 * rows * A if g.groups > 1 else rows * A  # one group: its stride is free
        assert args[8:12] == [G * rows * A, group, G * rows * A, group]
        assert args[12:17] == list(g)
        dense = R.outer_cross(l0.contiguous(), l1.contiguous(), h0.contiguous(), h1.contiguous(),
                              g, nb=1)
        assert torch.equal(got.data, dense.data)
        gi = R.to_ints(got)
        for q in range(3):
            want = _model(g, bits, xi[q, 0:2 * g.groups:2], xi[q, 1:2 * g.groups:2],
                          xi[q + 1, 0:2 * g.groups:2], xi[q + 1, 1:2 * g.groups:2])
            assert (gi[q] == want).all(), (device, bits, g, q)
        # L and H of different widths from two buffers, plain, without batch slots
        hb = R.from_ints(_rand(rng, (g.groups, rows, 3), bits), bits, device)
        g2 = R.OuterGeom(g.groups, rows, A, 3, 3 * A - 1)
        lo = R.outer_pairs(R.RT(buf.data[2], bits))[0]
        got, calls = _spied(monkeypatch, lambda: R.outer_cross(lo, None, hb, None, g2))  # noqa: B023
        assert calls[0][1][2] == lo.data.data_ptr() and calls[0][1][4] == hb.data.data_ptr()
        assert (R.to_ints(got) == _model(g2, bits, xi[2, 0:2 * g.groups:2], R.to_ints(hb))).all()


@pytest.mark.parametrize("bits", [64, 128])
def test_views_in_place_cpu(bits, monkeypatch):
    _check_views("cpu", bits, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [64, 128])
def test_views_in_place_gpu(bits, monkeypatch):
    _check_views("cuda:0", bits, monkeypatch)


def test_return_codes():
    """-3 malformed (n_out > A*B, n_out < 1, A or B < 1, negative sizes or strides, extents
    over slot_cap, one next component without the other), -2 a 1- or 4-byte element, 0 nothing
    to do; nothing is read in any of them."""
    L = nat.lib()
    bufs = [torch.zeros(64, dtype=torch.int64) for _ in range(5)]
    p = [nat.ptr(t) for t in bufs]

    def f(eb=8, slots=1, lst=8, lgr=8, hst=8, hgr=8, groups=1, rows=2, A=4, B=4, n_out=16,
          lb=p[1], hb=p[3]):
        return L.mx_outer_cross(0, eb, p[0], lb, p[2], hb, p[4], slots, lst, lgr, hst, hgr,
                                groups, rows, A, B, n_out, None)

    assert f() == 0 and f(lb=None, hb=None) == 0 and f(n_out=1) == 0
    assert f(eb=1) == -2 and f(eb=4) == -2
    assert f(rows=0) == 0 and f(groups=0) == 0 and f(slots=0) == 0
    for bad in (dict(n_out=17), dict(n_out=0), dict(n_out=-1), dict(A=0), dict(B=0), dict(A=-4),
                dict(B=-4), dict(rows=-1), dict(groups=-1), dict(slots=-1), dict(lst=-1),
                dict(lgr=-1), dict(hst=-1), dict(hgr=-1), dict(rows=1 << 31), dict(A=1 << 31),
                dict(lb=None), dict(hb=None),
                dict(slots=4, groups=1 << 30, rows=1 << 30, n_out=1),
                dict(slots=4, rows=1 << 30, A=1 << 30, n_out=1),
                dict(slots=4, rows=1 << 30, B=1 << 30, n_out=1)):
        assert f(**bad) == -3, bad
    # malformed before unsupported, as the other leaves
    assert f(eb=1, n_out=17) == -3
    for slots, far in ((4, 1 << 61), (3, (1 << 62) + 1)):
        for k in ("lst", "hst"):
            assert f(slots=slots, **{k: far}) == -3
        for k in ("lgr", "hgr"):
            assert f(slots=slots, groups=2, **{k: far}) == -3


def test_malformed_geometry_is_refused():
    x = R.from_ints(np.arange(8, dtype=object).reshape(1, 2, 4), 64, "cpu")
    for bad in (R.OuterGeom(1, 2, 4, 4, 17), R.OuterGeom(1, 2, 4, 4, 0), R.OuterGeom(1, 2, 0, 4, 1),
                R.OuterGeom(1, 2, 4, 2, 8), R.OuterGeom(2, 2, 4, 4, 16)):
        with pytest.raises(ValueError):
            R.outer_cross(x, None, x, None, bad)
    g = R.OuterGeom(1, 2, 4, 4, 16)
    with pytest.raises(ValueError, match="both operands or of neither"):
        R.outer_cross(x, x, x, None, g)
    bit = R.RT(torch.zeros((1, 2, 4), dtype=torch.uint8), 1)
    with pytest.raises(ValueError, match="arithmetic"):
        R.outer_cross(bit, None, bit, None, g)
    m = R.empty((3, 5, 2), 128, "meta")
    assert tuple(R.outer_cross(m, m, m, m, R.OuterGeom(3, 5, 2, 2, 3)).shape) == (3, 5, 3)


# ---------------------------------------------------------------------------
# the 64-bit index forms: two small slots 2^31 elements apart in one large device buffer
# ---------------------------------------------------------------------------
HEADROOM = 1 << 17  # fits32's headroom of the outer_cross launch (csrc/leaf_hip.hip)
BAND = 1 << 14      # words of defined data around each slot


@pytest.fixture(scope="module")
def far_buffer():
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    words = 2**32 + 2 * BAND  # 2^31 u128 elements
    need = words * 8 + (2 << 30)
    if free < need:
        pytest.skip(f"the far-stride buffer needs {need / 2**30:.2f} GiB of free device memory, "
                    f"{free / 2**30:.2f} GiB are free")
    buf = torch.empty(words, dtype=torch.int64, device="cuda:0")
    yield buf
    del buf
    torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["EDGE32", "EDGE64"])
@pytest.mark.parametrize("form", ["u64x2", "u64x1", "u128"])
def test_outer_index_forms(far_buffer, monkeypatch, form, which):
    """The last slot stride of the 32-bit forms and the first of the 64-bit ones, with the
    operands' slots far apart and L, H the paired groups of one state: bitwise the CPU twin and
    the dense device run."""
    bits, odd = (128, False) if form == "u128" else (64, form == "u64x1")
    w = bits // 64
    G, rows, A = 4, 17, 4
    g = R.OuterGeom(G // 2, rows, A, A, 13 if odd else 14)
    count = G * rows * A
    # an operand's reach from its own pointer: the last L group ends rows * A before the state
    # does, and H starts rows * A into it
    reach = count - rows * A
    first = 2**31 - HEADROOM - reach
    last = first - 1
    if form == "u64x2":  # an even stride on either side
        last, first = last - last % 2, first + first % 2
    stride = last if which == "EDGE32" else first
    assert (stride + reach < 2**31 - HEADROOM) == (which == "EDGE32")
    gen = torch.Generator().manual_seed(len(form) * 13 + len(which))

    def rnd(n):
        return torch.randint(-2**63, 2**63 - 1, (n,), dtype=torch.int64, generator=gen)

    for s in (0, stride * w):
        far_buffer[s:s + BAND] = rnd(BAND).to(far_buffer.device)
    tail = (2,) if w == 2 else ()
    dense = [rows * A * w, A * w, w] + ([1] if w == 2 else [])

    def view(off):
        assert off + (stride + count) * w <= far_buffer.numel() and off + count * w <= BAND
        return R.RT(far_buffer[off:].as_strided((2, G, rows, A) + tail, [stride * w] + dense), bits)

    a, b = view(0), view(4096)
    (la, ha), (lb, hb) = R.outer_pairs(a, nb=1), R.outer_pairs(b, nb=1)
    cpu = lambda t: R.RT(t.data.contiguous().cpu(), bits)  # noqa: E731
    for run in (lambda la, lb, ha, hb: R.outer_cross(la, lb, ha, hb, g, nb=1),
                lambda la, lb, ha, hb: R.outer_cross(la, None, ha, None, g, nb=1)):
        got, calls = _spied(monkeypatch, lambda: run(la, lb, ha, hb))  # noqa: B023
        # the far views reached the entry uncopied, at their strides: one launch, no dense copy
        assert [c[0] for c in calls] == ["mx_outer_cross"]
        args = calls[0][1]
        assert args[2] == la.data.data_ptr() and args[4] == ha.data.data_ptr()
        assert args[8:12] == [stride, 2 * rows * A, stride, 2 * rows * A]
        assert torch.equal(got.data.cpu(), run(cpu(la), cpu(lb), cpu(ha), cpu(hb)).data)
        assert torch.equal(got.data, run(la.contiguous(), lb.contiguous(), ha.contiguous(),
                                         hb.contiguous()).data)
