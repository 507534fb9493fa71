"""The prefix-sum leaf (mx_scan): R.scan against Python integers mod 2^64 / 2^128 for every
combination of ``exclusive`` and ``reverse``, on both sides of the chunk length (the one-launch
path, the three phases and their recursion), in place on slot views, against the torch
composition and the CPU twin; the return codes of the entry; the gfx950 kernel bitwise equal to
the CPU twin, its 64-bit index form included."""
import functools
import itertools

import numpy as np
import pytest
import torch

from moose_amd.ops import native as nat
from moose_amd.ops import ring as R

C = R.SCAN_CHUNK
# (outer, n, inner): single elements; odd rows; columns; 65 rows (crosses a 256-thread block);
# odd inner (the one-element u64 form); then both sides of one chunk and of two, with one and
# three lines in either position
SHAPES = ((1, 1, 1), (1, 2, 1), (1, 3, 2), (3, 5, 1), (1, 8, 3), (65, 8, 1), (2, 17, 5)) + tuple(
    s for n in (C - 1, C, C + 1, 2 * C + 1) for s in ((1, n, 1), (1, n, 3), (3, n, 1)))
ATTRS = tuple(itertools.product((False, True), (False, True)))  # (exclusive, reverse)


def _rand(rng, shape, bits):
    n = int(np.prod(shape))
    vals = [int.from_bytes(rng.bytes(bits // 8), "little") for _ in range(n)]
    return np.array(vals, dtype=object).reshape(shape)


def _model(x, bits, exclusive, reverse):
    """The prefix sums of an [outer, n, inner] array of Python integers."""
    a = x[:, ::-1] if reverse else x
    c = np.cumsum(a, axis=1)
    if exclusive:
        c = c - a
    c = c & ((1 << bits) - 1)
    return c[:, ::-1] if reverse else c


@functools.lru_cache(maxsize=None)
def _cases(bits):
    """(shape, input, {attrs: model}), computed once and shared by the CPU and GPU tests."""
    rng = np.random.default_rng(100 + bits)
    top = (1 << bits) - 1
    out = []
    for shape in SHAPES:
        x = _rand(rng, shape, bits)
        x[0, 0, 0] = top  # 2^bits - 1 and zero among the arbitrary ring values
        x[-1, -1, -1] = 0 if shape[1] > 1 else top
        xs = [x]
        if bits == 128:  # a line of 2^64 - 1: every step carries across the limb
            y = x.copy()
            y[0, :, 0] = (1 << 64) - 1
            xs.append(y)
        for v in xs:
            out.append((shape, v, {a: _model(v, bits, *a) for a in ATTRS}))
    return out


def test_chunk_and_workspace_agree_with_the_library():
    L = nat.lib()
    assert L.mx_scan_chunk() == C
    for slots, outer, n, inner in ((1, 1, C, 1), (1, 1, C + 1, 1), (3, 2, 2 * C + 1, 5),
                                   (4, 1, C * C + 1, 3), (1, 1, 1, 1)):
        assert L.mx_scan_ws_elems(slots, outer, n, inner) == R.scan_ws_elems(slots, outer, n, inner)
    assert R.scan_ws_elems(1, 1, C, 7) == 0 and R.scan_ws_elems(1, 1, C + 1, 1) == 4


@pytest.mark.parametrize("bits", [64, 128])
def test_scan_matches_python_integers_cpu(bits):
    for shape, x, want in _cases(bits):
        t = R.from_ints(x, bits, "cpu")
        for (ex, rev), w in want.items():
            g = R.ScanGeom(*shape, ex, rev)
            got = R.scan(t, g)
            assert tuple(got.shape) == shape
            assert (R.to_ints(got) == w).all(), ("scan", bits, g)
            assert (R.to_ints(R.scan_torch(t, g)) == w).all(), ("torch", bits, g)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [64, 128])
def test_scan_gpu_equals_cpu_bitwise(bits):
    for shape, x, want in _cases(bits):
        tc, tg = R.from_ints(x, bits, "cpu"), R.from_ints(x, bits, "cuda:0")
        for (ex, rev), w in want.items():
            g = R.ScanGeom(*shape, ex, rev)
            cpu, gpu = R.scan(tc, g), R.scan(tg, g)
            assert torch.equal(cpu.data, gpu.data.cpu()), ("gpu", bits, g)
            assert torch.equal(cpu.data, R.scan_torch(tg, g).data.cpu()), ("torch", bits, g)
        assert (R.to_ints(gpu) == w).all()


def _check_two_levels(device):
    """An axis of more than SCAN_CHUNK^2 positions: the chunk sums take three phases too."""
    n = C * C + C + 1
    rng = np.random.default_rng(3)
    v = rng.integers(0, 1 << 64, size=(1, n, 2), dtype=np.uint64)
    for ex, rev in ATTRS:
        a = v[:, ::-1] if rev else v
        want = np.cumsum(a, axis=1, dtype=np.uint64)
        want = (want - a if ex else want)
        want = want[:, ::-1] if rev else want
        g = R.ScanGeom(1, n, 2, ex, rev)
        got = R.scan(R.RT(torch.from_numpy(v.view(np.int64)).to(device), 64), g)
        assert np.array_equal(got.data.cpu().numpy().view(np.uint64), want), (device, g)
    # Z_2^128 with a carry at every step, against the closed form (t + 1) * (2^64 - 1)
    x = np.full((1, n, 1), (1 << 64) - 1, dtype=object)
    got = R.to_ints(R.scan(R.from_ints(x, 128, device), R.ScanGeom(1, n, 1)))
    assert all(int(got[0, t, 0]) == (t + 1) * ((1 << 64) - 1) for t in (0, 1, C, n // 2, n - 1))
    assert (np.diff(got[0, :, 0]) == (1 << 64) - 1).all()


def test_two_levels_of_chunks_cpu():
    _check_two_levels("cpu")


@pytest.mark.gpu
def test_two_levels_of_chunks_gpu():
    _check_two_levels("cuda:0")


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


def _check_views(device, bits, monkeypatch):
    rng = np.random.default_rng(17 + bits)
    for shape, (ex, rev) in (((3, 5, 1), (False, False)), ((1, 8, 3), (True, True)),
                             ((2, 17, 5), (False, True)), ((1, 2 * C + 1, 2), (True, False))):
        g = R.ScanGeom(*shape, ex, rev)
        xi = _rand(rng, (4,) + shape, bits)
        buf = R.from_ints(xi, bits, device)
        s0, s1 = R.RT(buf.data[0:3], bits), R.RT(buf.data[1:4], bits)
        wide = R.RT(R.from_ints(_rand(rng, (6,) + shape, bits), bits, device).data[::2], bits)
        count = int(np.prod(shape))
        for v, stride in ((s0, count), (s1, count), (wide, 2 * count)):
            spy = _Spy(nat.lib())
            with monkeypatch.context() as m:
                m.setattr(nat, "lib", lambda: spy)  # noqa: B023
                got = R.scan(v, g, nb=1)
            # the view went through uncopied, at its slot stride
            assert [c[0] for c in spy.calls] == ["mx_scan"]
            assert v.data.data_ptr() in spy.calls[0][1] and stride in spy.calls[0][1]
            assert torch.equal(got.data, R.scan(v.contiguous(), g, nb=1).data), (device, bits, g)
        all4 = R.to_ints(R.scan(buf, g, nb=1))
        for q in range(4):
            assert (all4[q] == _model(xi[q], bits, ex, rev)).all(), (device, bits, g, q)


@pytest.mark.parametrize("bits", [64, 128])
def test_slot_views_in_place_cpu(bits, monkeypatch):
    _check_views("cpu", bits, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [64, 128])
def test_slot_views_in_place_gpu(bits, monkeypatch):
    _check_views("cuda:0", bits, monkeypatch)


def test_return_codes():
    """-3 malformed (negative extents, an extent or stride over slot_cap, a short workspace),
    -2 a 4-byte element, 0 nothing to do; nothing is read in any of them."""
    L = nat.lib()
    x, out, ws = (torch.zeros(4 * C, dtype=torch.int64) for _ in range(3))
    p = [nat.ptr(t) for t in (x, out, ws)]

    def scan(eb=8, slots=1, xst=8, outer=1, n=8, inner=1, ws=None, nws=0):
        return L.mx_scan(0, eb, p[0], p[1], ws, nws, slots, xst, outer, n, inner, 0, 0, None)

    assert scan() == 0 and out.eq(0).all()
    assert scan(eb=4) == -2
    assert scan(outer=0) == 0 and scan(n=0) == 0 and scan(inner=0) == 0 and scan(slots=0) == 0
    for bad in (dict(outer=-1), dict(n=-1), dict(inner=-1), dict(slots=-1), dict(xst=-1),
                dict(n=1 << 31), dict(slots=4, xst=1 << 61), dict(slots=3, xst=(1 << 62) + 1),
                dict(slots=4, outer=1 << 30, n=1 << 30)):
        assert scan(**bad) == -3, bad
    assert L.mx_scan_ws_elems(1, -1, 8, 1) == -3
    # an axis of more than one chunk needs its workspace
    long = dict(n=C + 1, xst=C + 1)
    assert scan(**long) == -3 and scan(ws=p[2], nws=3, **long) == -3
    assert scan(ws=p[2], nws=4, **long) == 0


def test_malformed_operands_are_refused():
    x = R.from_ints(np.arange(8, dtype=object), 64, "cpu")
    for bad in (R.ScanGeom(1, 6, 1), R.ScanGeom(2, 8, 1), R.ScanGeom(-1, -8, 1)):
        with pytest.raises(ValueError):
            R.scan(x, bad)
    with pytest.raises(ValueError):
        R.scan(R.RT(torch.zeros(8, dtype=torch.uint8), 1), R.ScanGeom(1, 8, 1))
    assert tuple(R.scan(R.empty((3, 0, 2), 64, "cpu"), R.ScanGeom(3, 0, 2)).shape) == (3, 0, 2)
    meta = R.scan(R.empty((2, 3, 4), 128, "meta"), R.ScanGeom(2, 3, 4, True, True))
    assert tuple(meta.shape) == (2, 3, 4) and meta.device.type == "meta"


# ---------------------------------------------------------------------------
# the 64-bit index form: two small slots 2^31 elements apart in one large device buffer
# ---------------------------------------------------------------------------
HEADROOM = 1 << 17  # fits32's headroom of the scan launches (csrc/leaf_hip.hip)
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
def test_scan_index_forms(far_buffer, monkeypatch, form, which):
    """The last slot stride of the 32-bit form and the first of the 64-bit one, through all
    three phases: bitwise the CPU twin and the dense device run."""
    bits, odd = (128, False) if form == "u128" else (64, form == "u64x1")
    w = bits // 64
    shape = (2, 2 * C + 1, 3 if odd else 2)
    count = int(np.prod(shape))
    last = 2**31 - HEADROOM - 1 - count
    first = last + 1
    if form == "u64x2":  # an even stride on either side
        last, first = last - last % 2, first + first % 2
    stride = last if which == "EDGE32" else first
    assert (stride + count < 2**31 - HEADROOM) == (which == "EDGE32")
    gen = torch.Generator().manual_seed(len(form) * 7 + len(which))
    off = 1 if odd else 0
    for s in (0, stride * w):
        far_buffer[s:s + BAND] = torch.randint(-2**63, 2**63 - 1, (BAND,), dtype=torch.int64,
                                               generator=gen).to(far_buffer.device)
    assert off + (stride + count) * w <= far_buffer.numel() and count * w + off <= BAND
    tail = (2,) if w == 2 else ()
    dense = [shape[1] * shape[2] * w, shape[2] * w, w] + ([1] if w == 2 else [])
    view = R.RT(far_buffer[off:].as_strided((2,) + shape + tail, [stride * w] + dense), bits)
    for ex, rev in ((False, False), (True, True)):
        g = R.ScanGeom(*shape, ex, rev)
        spy = _Spy(nat.lib())
        with monkeypatch.context() as m:
            m.setattr(nat, "lib", lambda: spy)  # noqa: B023
            got = R.scan(view, g, nb=1)
        assert view.data.data_ptr() in spy.calls[0][1] and stride in spy.calls[0][1]
        copy = view.contiguous()
        assert torch.equal(got.data.cpu(), R.scan(R.RT(copy.data.cpu(), bits), g, nb=1).data)
        assert torch.equal(got.data, R.scan(copy, g, nb=1).data)
