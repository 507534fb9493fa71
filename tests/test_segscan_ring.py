"""The segmented-scan leaves (mx_segscan_cross / _apply): R.segscan_cross and R.segscan_apply
against Python integers mod 2^64 / 2^128 at every stage offset of small scans and at j = n - 1,
with arbitrary ring values as flags (the kernels are ring-linear), in place on slot views,
against the torch compositions, and as a whole segmented scan run in the clear; the return
codes of the entries; the gfx950 kernels bitwise equal to the CPU twins, their 64-bit index
forms included."""
import functools

import numpy as np
import pytest
import torch

from moose_amd.ops import native as nat
from moose_amd.ops import ring as R

# (outer, n, inner): two positions; an odd axis with a value column; odd rows of flags only;
# columns; 65 rows (crosses a 256-thread block); odd inner (the one-element u64 form); a
# longer even one
SHAPES = ((1, 2, 1), (1, 3, 2), (3, 5, 1), (1, 8, 3), (65, 8, 1), (2, 17, 5), (2, 64, 4))


def _rand(rng, shape, bits):
    n = int(np.prod(shape))
    vals = [int.from_bytes(rng.bytes(bits // 8), "little") for _ in range(n)]
    return np.array(vals, dtype=object).reshape(shape)


def _offsets(n):
    return sorted(set(R.segscan_stages(n)) | {n - 1})


def _model(j, bits, a, b=None, p=None):
    """(cross, apply) of stage j in Python integers on [outer, n, inner] arrays."""
    M = (1 << bits) - 1
    n = a.shape[1]
    ga, ta = a[:, j:, -1:], a[:, :n - j]
    if b is None:
        cross = (ga * ta) & M
    else:
        cross = (ga * (ta + b[:, :n - j]) + b[:, j:, -1:] * ta) & M
    out = None
    if p is not None:
        out = a.copy()
        out[:, j:, :-1] = (a[:, j:, :-1] + p[:, :, :-1]) & M
        out[:, j:, -1] = p[:, :, -1]
    return cross, out


@functools.lru_cache(maxsize=None)
def _cases(bits):
    """(geometry, inputs, model results), computed once and shared by the CPU and GPU tests."""
    rng = np.random.default_rng(200 + bits)
    top = (1 << bits) - 1
    out = []
    for outer, n, inner in SHAPES:
        a, b = _rand(rng, (outer, n, inner), bits), _rand(rng, (outer, n, inner), bits)
        a[0, 0, 0], a[0, 1, -1], b[-1, -1, -1], b[0, 0, -1] = top, top, 0, 0
        for j in _offsets(n):
            p = _rand(rng, (outer, n - j, inner), bits)
            p[0, 0, 0], p[-1, -1, -1] = top, 0
            g = R.SegscanGeom(outer, n, inner, j)
            cross, app = _model(j, bits, a, b, p)
            out.append((g, a, b, p, cross, app, _model(j, bits, a)[0]))
    return out


def test_stage_offsets():
    assert R.segscan_stages(1) == [] and R.segscan_stages(2) == [1]
    assert R.segscan_stages(5) == [1, 2, 4] and R.segscan_stages(8) == [1, 2, 4]
    assert R.segscan_stages(17) == [1, 2, 4, 8, 16]
    assert all(len(R.segscan_stages(n)) == (n - 1).bit_length() for n in range(1, 70))


def _leaves(g, t, a, b, p):
    return (R.segscan_cross(t(a), t(b), g), R.segscan_apply(t(a), t(p), g),
            R.segscan_cross(t(a), None, g))


@pytest.mark.parametrize("bits", [64, 128])
def test_leaves_match_python_integers_cpu(bits):
    t = lambda v: R.from_ints(v, bits, "cpu")  # noqa: E731
    for g, a, b, p, cross, app, plain in _cases(bits):
        c, o, pl = _leaves(g, t, a, b, p)
        assert tuple(c.shape) == cross.shape and tuple(o.shape) == a.shape
        assert (R.to_ints(c) == cross).all(), ("cross", bits, g)
        assert (R.to_ints(o) == app).all(), ("apply", bits, g)
        assert (R.to_ints(pl) == plain).all(), ("plain", bits, g)
        # plain mode = cross mode with a zero next component
        assert torch.equal(R.segscan_cross(t(a), t(np.zeros_like(b)), g).data, pl.data)
        assert (R.to_ints(R.segscan_cross_torch(t(a), t(b), g)) == cross).all(), ("torch", g)
        assert (R.to_ints(R.segscan_cross_torch(t(a), None, g)) == plain).all(), ("torch", g)
        assert (R.to_ints(R.segscan_apply_torch(t(a), t(p), g)) == app).all(), ("torch", g)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [64, 128])
def test_leaves_gpu_equal_cpu_bitwise(bits):
    tc = lambda v: R.from_ints(v, bits, "cpu")  # noqa: E731
    uploaded = {}

    def tg(v):  # one upload per array
        if id(v) not in uploaded:
            uploaded[id(v)] = R.from_ints(v, bits, "cuda:0")
        return uploaded[id(v)]

    for g, a, b, p, _cross, _app, _plain in _cases(bits):
        cpu, gpu = _leaves(g, tc, a, b, p), _leaves(g, tg, a, b, p)
        tor = (R.segscan_cross_torch(tg(a), tg(b), g), R.segscan_apply_torch(tg(a), tg(p), g),
               R.segscan_cross_torch(tg(a), None, g))
        for name, x, y, z in zip(("cross", "apply", "plain"), cpu, gpu, tor):
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
    rng = np.random.default_rng(23 + bits)
    for (outer, n, inner), j in (((3, 5, 1), 2), ((1, 8, 3), 4), ((2, 17, 5), 16), ((2, 64, 4), 1)):
        g = R.SegscanGeom(outer, n, inner, j)
        xi, pi = _rand(rng, (4, outer, n, inner), bits), _rand(rng, (4, outer, n - j, inner), bits)
        xbuf, pbuf = R.from_ints(xi, bits, device), R.from_ints(pi, bits, device)
        x0, x1 = R.RT(xbuf.data[0:3], bits), R.RT(xbuf.data[1:4], bits)
        p0, p1 = R.RT(pbuf.data[0:3], bits), R.RT(pbuf.data[1:4], bits)
        assert x0.data.untyped_storage().data_ptr() == x1.data.untyped_storage().data_ptr()
        nx, np_ = outer * n * inner, outer * (n - j) * inner
        cross, calls = _spied(monkeypatch, lambda: R.segscan_cross(x0, x1, g, nb=1))  # noqa: B023
        assert [c[0] for c in calls] == ["mx_segscan_cross"]  # both views uncopied, one stride
        assert x0.data.data_ptr() in calls[0][1] and x1.data.data_ptr() in calls[0][1]
        assert nx in calls[0][1]
        assert torch.equal(cross.data, R.segscan_cross(x0.clone(), x1.clone(), g, nb=1).data)
        app4, calls = _spied(monkeypatch, lambda: R.segscan_apply(xbuf, pbuf, g, nb=1))  # noqa: B023
        for lo, xv, pv in ((0, x0, p0), (1, x1, p1)):
            got, calls = _spied(monkeypatch, lambda: R.segscan_apply(xv, pv, g, nb=1))  # noqa: B023
            assert xv.data.data_ptr() in calls[0][1] and pv.data.data_ptr() in calls[0][1]
            assert torch.equal(got.data, app4.data[lo:lo + 3])
        cg, ag = R.to_ints(cross), R.to_ints(app4)
        for q in range(4):
            want = _model(j, bits, xi[q], xi[min(q + 1, 3)], pi[q])
            assert (ag[q] == want[1]).all(), (device, bits, g, q)
            if q < 3:
                assert (cg[q] == want[0]).all(), (device, bits, g, q)
        # a slot stride larger than the slot: every other slot of a wider buffer
        wide = R.RT(R.from_ints(_rand(rng, (6, outer, n, inner), bits), bits, device).data[::2], bits)
        got, calls = _spied(monkeypatch, lambda: R.segscan_cross(wide, None, g, nb=1))  # noqa: B023
        assert wide.data.data_ptr() in calls[0][1] and 2 * nx in calls[0][1]
        assert torch.equal(got.data, R.segscan_cross(wide.contiguous(), None, g, nb=1).data)
        got, calls = _spied(monkeypatch, lambda: R.segscan_apply(wide, p0, g, nb=1))  # noqa: B023
        assert 2 * nx in calls[0][1] and np_ in calls[0][1]
        assert torch.equal(got.data, R.segscan_apply(wide.contiguous(), p0, g, nb=1).data)


@pytest.mark.parametrize("bits", [64, 128])
def test_slot_views_in_place_cpu(bits, monkeypatch):
    _check_views("cpu", bits, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [64, 128])
def test_slot_views_in_place_gpu(bits, monkeypatch):
    _check_views("cuda:0", bits, monkeypatch)


def _scan_in_the_clear(device, bits, outer, n, cols, rng):
    """Every stage as plain cross -> apply on ordinary integers with 0/1 flags: the inclusive
    segmented prefix sums, and the flag column zero below j after the stage of offset j."""
    vals = rng.integers(-1000, 1000, size=(outer, n, cols))
    flags = rng.integers(0, 2, size=(outer, n, 1))
    flags[:, 0] = 0
    state = np.concatenate([vals, flags], axis=2)
    x = R.from_ints(np.vectorize(lambda v: int(v) % (1 << bits), otypes=[object])(state), bits,
                    device)
    for j in R.segscan_stages(n):
        g = R.SegscanGeom(outer, n, cols + 1, j)
        x = R.segscan_apply(x, R.segscan_cross(x, None, g), g)
        assert (R.to_ints(x)[:, :min(2 * j, n), -1] == 0).all()
    want = np.zeros_like(vals)
    for o in range(outer):
        for i in range(n):
            want[o, i] = vals[o, i] + (want[o, i - 1] if flags[o, i, 0] else 0)
    got = R.to_signed_ints(x).astype(np.int64)
    assert (got[:, :, :-1] == want).all() and (got[:, :, -1] == 0).all(), (device, bits, n, cols)


def _check_whole_scan(device):
    rng = np.random.default_rng(9)
    for bits in (64, 128):
        for n in (1, 2, 3, 5, 8, 17, 64):
            _scan_in_the_clear(device, bits, 2, n, 1, rng)
        _scan_in_the_clear(device, bits, 1, 17, 3, rng)


def test_segmented_scan_in_the_clear_cpu():
    _check_whole_scan("cpu")


@pytest.mark.gpu
def test_segmented_scan_in_the_clear_gpu():
    _check_whole_scan("cuda:0")


def test_return_codes():
    """-3 malformed (j < 1, j >= n, negative extents, an extent or stride over slot_cap), -2 a
    4-byte element, 0 nothing to do; nothing is read in any of them."""
    L = nat.lib()
    bufs = [torch.zeros(64, dtype=torch.int64) for _ in range(4)]
    p = [nat.ptr(t) for t in bufs]

    def cross(eb=8, slots=1, st=8, outer=1, n=8, inner=1, j=1):
        return L.mx_segscan_cross(0, eb, p[0], p[1], p[3], slots, st, outer, n, inner, j, None)

    def apply(eb=8, slots=1, xst=8, pst=8, outer=1, n=8, inner=1, j=1):
        return L.mx_segscan_apply(0, eb, p[0], p[2], p[3], slots, xst, pst, outer, n, inner, j,
                                  None)

    for f in (cross, apply):
        assert f() == 0
        assert f(eb=4) == -2
        assert f(outer=0) == 0 and f(inner=0) == 0 and f(slots=0) == 0
        for bad in (dict(j=0), dict(j=-1), dict(j=8), dict(j=9), dict(n=0), dict(n=1),
                    dict(outer=-1), dict(inner=-1), dict(n=-8), dict(slots=-1),
                    dict(n=1 << 31), dict(slots=4, outer=1 << 30, n=1 << 30)):
            assert f(**bad) == -3, (f.__name__, bad)
    for slots, far in ((4, 1 << 61), (3, (1 << 62) + 1)):
        assert cross(slots=slots, st=far) == -3
        assert apply(slots=slots, xst=far) == -3 and apply(slots=slots, pst=far) == -3
    assert cross(st=-1) == -3 and apply(xst=-1) == -3 and apply(pst=-1) == -3


def test_malformed_stage_is_refused():
    x = R.from_ints(np.arange(8, dtype=object), 64, "cpu")
    for bad in (R.SegscanGeom(1, 8, 1, 0), R.SegscanGeom(1, 8, 1, 8), R.SegscanGeom(1, 6, 1, 1),
                R.SegscanGeom(2, 8, 1, 1)):
        with pytest.raises(ValueError):
            R.segscan_cross(x, None, bad)
    with pytest.raises(ValueError):
        R.segscan_apply(x, x, R.SegscanGeom(1, 8, 1, 1))  # the products hold n - j positions
    g = R.SegscanGeom(2, 5, 3, 2)
    m = R.empty((2, 5, 3), 128, "meta")
    assert tuple(R.segscan_cross(m, m, g).shape) == (2, 3, 3)
    assert tuple(R.segscan_apply(m, R.empty((2, 3, 3), 128, "meta"), g).shape) == (2, 5, 3)


# ---------------------------------------------------------------------------
# the 64-bit index forms: two small slots 2^31 elements apart in one large device buffer
# ---------------------------------------------------------------------------
HEADROOM = 1 << 17  # fits32's headroom of the segscan launches (csrc/leaf_hip.hip)
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
def test_segscan_index_forms(far_buffer, monkeypatch, form, which):
    """The last slot stride of the 32-bit forms and the first of the 64-bit ones, with the
    state far apart: bitwise the CPU twins and the dense device runs."""
    bits, odd = (128, False) if form == "u128" else (64, form == "u64x1")
    w = bits // 64
    shape = (2, 17, 5 if odd else 4)
    g = R.SegscanGeom(*shape, 4)
    count = int(np.prod(shape))
    last = 2**31 - HEADROOM - 1 - count
    first = last + 1
    if form == "u64x2":  # an even stride on either side
        last, first = last - last % 2, first + first % 2
    stride = last if which == "EDGE32" else first
    assert (stride + count < 2**31 - HEADROOM) == (which == "EDGE32")
    gen = torch.Generator().manual_seed(len(form) * 11 + len(which))

    def rnd(n):
        return torch.randint(-2**63, 2**63 - 1, (n,), dtype=torch.int64, generator=gen)

    for s in (0, stride * w):
        far_buffer[s:s + BAND] = rnd(BAND).to(far_buffer.device)
    tail = (2,) if w == 2 else ()
    dense = [shape[1] * shape[2] * w, shape[2] * w, w] + ([1] if w == 2 else [])

    def view(off):
        assert off + (stride + count) * w <= far_buffer.numel() and off + count * w <= BAND
        return R.RT(far_buffer[off:].as_strided((2,) + shape + tail, [stride * w] + dense), bits)

    off = 1 if odd else 0
    a, b = view(off), view(off + 4096)
    p = R.RT(rnd(2 * (shape[1] - g.j) * shape[0] * shape[2] * w).reshape(
        (2, shape[0], shape[1] - g.j, shape[2]) + tail).to(far_buffer.device), bits)
    cpu = lambda t: R.RT(t.data.contiguous().cpu(), bits)  # noqa: E731
    for entry, run in (("mx_segscan_cross", lambda a, b, p: R.segscan_cross(a, b, g, nb=1)),
                       ("mx_segscan_cross", lambda a, b, p: R.segscan_cross(a, None, g, nb=1)),
                       ("mx_segscan_apply", lambda a, b, p: R.segscan_apply(a, p, g, nb=1))):
        got, calls = _spied(monkeypatch, lambda: run(a, b, p))  # noqa: B023
        # the far views reached the entry uncopied, at their stride: one launch, no dense copy
        assert [c[0] for c in calls] == [entry]
        assert a.data.data_ptr() in calls[0][1] and stride in calls[0][1]
        assert torch.equal(got.data.cpu(), run(cpu(a), cpu(b), cpu(p)).data)
        assert torch.equal(got.data, run(a.contiguous(), b.contiguous(), p).data)
