"""The index-width switch of the leaf kernels (csrc/leaf_hip.hip): every family is a template
over an index type, ``int32_t`` while ``fits32(headroom, {extents})`` holds and ``int64_t``
beyond, and every extent is ``(slots - 1) * slot_stride + n``.  The wrappers of
``moose_amd.ops.ring`` read a ``[slots, ...]`` view with dense slots in place, so two small
slots that lie 2^31 elements or more apart in one large, mostly untouched device buffer take
the 64-bit form and put real offsets above 2^31 and 2^32 through every ``blockIdx.z * slot
stride`` of the kernels -- no 2^31 elements of data are needed.  The same views reach the
32-bit form at the largest extent ``fits32`` lets it have.

Each case runs a wrapper on views at three slot strides -- EDGE32, the last 32-bit launch;
EDGE64, the first 64-bit one; FAR, above 2^32 words -- and compares bit for bit with the CPU
twin on a dense stack of the two slots (which the per-family test files pin to independent
integer models) and with the device kernel on a dense device copy (the 32-bit form).  These
are exact ring operations: no tolerance anywhere.

What this does not reach: output extents of 2^31 elements or more need real data of that
size, so the 64-bit forms run with small ``rows``, ``K`` and ``n_out`` only."""
import ctypes
import math

import pytest
import torch

from moose_amd.ops import native as nat
from moose_amd.ops import ring as R

W = 2**32 + 4112  # FAR: the slot stride in int64 words (even: W // 2 u128 elements)
TAIL = 2**22      # words behind slot 1's start at the FAR stride
BAND = 1 << 16    # words (bytes for a bit tensor) of defined random data around slot 0 and slot 1
BASE = 4096       # offset of a case's first operand inside a band; the operands are
SPACING = 6144    # SPACING apart and hold at most SLOT_MAX words (bytes) each
SLOT_MAX = 4096
# A u64 stride of W truncated to 32 bits is 4112: slot 1 would be read at BASE + 4112 + i of the
# band around slot 0 -- defined data that differs -- so a narrowed stride fails by comparison and
# does not fault.  The u128 stride, W // 2 = 2^31 + 2056 elements, cannot be protected this way
# without doubling the buffer: its low 32 bits are a negative int32, and 2^32 more words
# would have to lie in front of slot 0.

# fits32's headroom per leaf (the mxh_* entries at the end of leaf_hip.hip): the overshoot a
# lane's last loop step may add to an index
HEADROOM_ROWS = 1 << 17    # im2col, perm_gather: at most 65,536 rows of grid per step
HEADROOM_LANES = 1 << 23   # the rest: at most 2048 blocks x 256 lanes x 2 elements per step
WIDTH_LIMIT = 2**31

EDGE32, EDGE64, FAR = "EDGE32", "EDGE64", "FAR"
STRIDES = (EDGE32, EDGE64, FAR)
# u64x2: two u64 per lane (even inner extent, even stride, 16-byte-aligned base); u64x1: one
# per lane (odd inner extent and an odd base offset); u128; u8: im2col's bit tensors
U64X2, U64X1, U128, U8 = "u64x2", "u64x1", "u128", "u8"
BITS = {U64X2: 64, U64X1: 64, U128: 128, U8: 1}


def fits32(headroom, extents):
    """leaf_hip.hip's fits32: 32-bit indices while every extent is below 2^31 - headroom."""
    return all(e < WIDTH_LIMIT - headroom for e in extents)


def edge_strides(count, headroom, even=False):
    """(EDGE32, EDGE64) for two slots of ``count`` elements: the largest slot stride whose
    extent ``stride + count`` is at most 2^31 - headroom - 1, and the smallest one whose
    extent is at least 2^31 - headroom; both even where the form under test needs it."""
    last = WIDTH_LIMIT - headroom - 1 - count
    first = last + 1
    if even:
        last -= last % 2
        first += first % 2
    return last, first


# ---------------------------------------------------------------------------
# CPU-only checks of the arithmetic and of the operand helper
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("headroom", [HEADROOM_ROWS, HEADROOM_LANES])
@pytest.mark.parametrize("count", [1, 60, 257, 4096])
@pytest.mark.parametrize("even", [False, True])
def test_edge_strides_sit_on_both_sides_of_fits32(headroom, count, even):
    assert fits32(headroom, [WIDTH_LIMIT - headroom - 1])
    assert not fits32(headroom, [WIDTH_LIMIT - headroom])
    last, first = edge_strides(count, headroom, even)
    assert fits32(headroom, [last + count]) and not fits32(headroom, [first + count])
    # neighbours among the admissible strides: nothing lies between the two
    assert first - last == (2 if even else 1)
    if even:
        assert last % 2 == 0 and first % 2 == 0
    else:  # the extents are the boundary values themselves
        assert last + count == WIDTH_LIMIT - headroom - 1 and first + count == WIDTH_LIMIT - headroom
    assert not fits32(headroom, [W // 2 + count])


@pytest.mark.parametrize("bits", [64, 128])
def test_leaf_operand_keeps_a_far_stride_exactly(bits):
    w = bits // 64
    tail = (2,) if w == 2 else ()
    words = torch.empty(W + TAIL, dtype=torch.int64, device="meta")
    view = words[BASE:].as_strided((2, 5, 6) + tail, (W, 6 * w, w) + ((1,) if w == 2 else ()))
    d, st = R._leaf_operand(R.RT(view, bits), 1, 30)
    assert st == W // w and d is view and d.stride(0) == W and d.storage_offset() == BASE
    if w == 2:  # an odd word stride is no whole number of u128 elements: a dense copy
        odd = words[BASE:].as_strided((2, 5, 6, 2), (W + 1, 12, 2, 1))
        d, st = R._leaf_operand(R.RT(odd, bits), 1, 30)
        assert st == 30 and d.is_contiguous() and d is not odd


# ---------------------------------------------------------------------------
# the shared buffer
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def far_buffer():
    """One device tensor of W + TAIL int64 words (about 32 GiB), never filled as a whole."""
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    need = (W + TAIL) * 8 + (2 << 30)
    print(f"\nleaf index forms: {free / 2**30:.2f} GiB of device memory free, "
          f"{need / 2**30:.2f} GiB needed")
    if free < need:
        pytest.skip(f"the far-stride buffer needs {need / 2**30:.2f} GiB of free device memory, "
                    f"{free / 2**30:.2f} GiB are free")
    buf = torch.empty(W + TAIL, dtype=torch.int64, device="cuda:0")
    yield buf
    del buf
    torch.cuda.empty_cache()


class _Spy:
    """nat.lib() with every call recorded as (name, flat arguments)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            flat = []
            for a in args:
                flat.extend(list(a) if isinstance(a, ctypes.Array) else [a])
            self.calls.append((name, flat))
            return fn(*args)

        return call


def _random(shape, bits, gen):
    if bits == 1:
        return torch.randint(0, 256, shape, dtype=torch.uint8, generator=gen)
    return torch.randint(-2**63, 2**63 - 1, shape, dtype=torch.int64, generator=gen)


def _dense_strides(shape):
    out, acc = [], 1
    for s in reversed(shape):
        out.append(acc)
        acc *= s
    return tuple(reversed(out))


def _check(buf, monkeypatch, case, form, which):
    bits = BITS[form]
    w = 2 if bits == 128 else 1              # int64 words (bytes for bits) per element
    odd, even = form == U64X1, form == U64X2
    specs, run = case["make"](odd, bits)     # [(name, slot shape, kind)], run(ops, device)
    headroom = case["headroom"]
    count = {name: math.prod(shape) for name, shape, _ in specs}
    far_count = {count[name] for name, _, kind in specs if kind == "far"}
    assert len(far_count) == 1               # the members of a far pair are one size
    far_count = far_count.pop()
    last, first = edge_strides(far_count, headroom, even)
    stride = {EDGE32: last, EDGE64: first, FAR: W // w}[which]  # in elements
    if even:
        assert stride % 2 == 0
    # which side of the threshold the launch is meant to fall on, by plain arithmetic
    extents, strides = [], {}
    for name, shape, kind in specs:
        strides[name] = {"far": stride, "dense": count[name],
                         "edge64": edge_strides(count[name], headroom, even)[1]}[kind]
        extents.append(strides[name] + count[name])
    small = which == EDGE32 and all(kind != "edge64" for _, _, kind in specs)
    assert fits32(headroom, extents) == small
    slack = 1 if even else 0  # an even stride may miss the boundary value by one
    if which == EDGE32:
        assert 0 <= (WIDTH_LIMIT - headroom - 1) - (stride + far_count) <= slack
    elif which == EDGE64:
        assert 0 <= (stride + far_count) - (WIDTH_LIMIT - headroom) <= slack
    else:
        assert stride * w == W and (bits != 64 or stride > 2**32)

    flat = buf.view(torch.uint8) if bits == 1 else buf
    gen = torch.Generator().manual_seed(sum(map(ord, case["id"] + form + which)))
    # defined random data around slot 0 and around slot 1 of every stride in use
    for s in {0} | {strides[name] * w for name, _, kind in specs if kind != "dense"}:
        flat[s:s + BAND] = _random((BAND,), bits, gen).to(buf.device)
    ops, views = {}, []
    for i, (name, shape, kind) in enumerate(specs):
        tail = (2,) if bits == 128 else ()
        if kind == "dense":
            ops[name] = R.RT(_random((2,) + shape + tail, bits, gen).to(buf.device), bits)
            continue
        off = BASE + i * SPACING + (1 if odd else 0)
        assert count[name] * w <= SLOT_MAX and off + SLOT_MAX + 4112 <= BAND
        assert off + strides[name] * w + count[name] * w <= flat.numel()  # slot 1 ends inside
        v = flat[off:].as_strided((2,) + shape + tail,
                                  (strides[name] * w,) + _dense_strides(shape + tail))
        assert (v.data_ptr() % 16 == 0) == (not odd)
        ops[name] = R.RT(v, bits)
        views.append(name)

    spy = _Spy(nat.lib())
    with monkeypatch.context() as m:
        m.setattr(nat, "lib", lambda: spy)
        got = run(ops, buf.device)
    # the wrapper passed every view through in place, at its stride: one launch, no copy
    assert [name for name, _ in spy.calls] == [case["entry"]]
    args = spy.calls[0][1]
    for name in views:
        assert ops[name].data.data_ptr() in args and strides[name] in args, (name, strides[name])

    dense = {name: R.RT(t.data.contiguous(), bits) for name, t in ops.items()}
    assert all(t.data.is_contiguous() and t.data.data_ptr() != ops[name].data.data_ptr()
               for name, t in dense.items() if name in views)
    want = run({name: R.RT(t.data.cpu(), bits) for name, t in dense.items()}, torch.device("cpu"))
    assert torch.equal(got.data.cpu(), want.data), "strided device run != CPU twin"
    assert torch.equal(got.data, run(dense, buf.device).data), "strided != dense device run"


# ---------------------------------------------------------------------------
# the cases: one non-trivial small problem per family, from the family's own test file
# ---------------------------------------------------------------------------
CASES = []


def _case(id, entry, headroom, make, forms=(U64X2, U64X1, U128)):  # noqa: A002
    CASES.extend(pytest.param(dict(id=id, entry=entry, headroom=headroom, make=make), form, which,
                              id=f"{id}-{form}-{which}") for form in forms for which in STRIDES)


# a 3 x 3 window with padding, stride 2 on the height and dilation 2 on the width, N = 2
_WIN = dict(kernel_shape=(3, 3), strides=(2, 1), pads=(1, 0, 1, 2), dilations=(1, 2))
_IMG_H = 5


def _image(N, C, H, Wd, fmt):
    return (N, C, H, Wd) if fmt == "NCHW" else (N, H, Wd, C)


def _im2col_case(fmt):
    def make(odd, bits):  # K = 9 C: even with C = 2
        shape = _image(2, 3 if odd else 2, _IMG_H, 6, fmt)
        return [("a", shape, "far")], lambda ops, dev: R.im2col(ops["a"], data_format=fmt, nb=1,
                                                                **_WIN)
    return make


def _col2im_case(fmt):
    def make(odd, bits):  # inner: C (NHWC) or W (NCHW)
        C, Wd = (3, 5) if odd else (2, 6)
        OH, OW = R.im2col_geometry(_image(2, C, _IMG_H, Wd, fmt), data_format=fmt, **_WIN)[14:16]
        return ([("a", (2 * OH * OW, C * 9), "far")],
                lambda ops, dev: R.col2im(ops["a"], (C, _IMG_H, Wd), data_format=fmt, nb=1, **_WIN))
    return make


def _resize_case(fmt, mode):
    def make(odd, bits):  # inner: C (NHWC) or OW (NCHW, always one element per lane)
        C, OW = (3, 7) if odd else (2, 6)
        wb = (R.resize_weight_bits(4, 7, mode), R.resize_weight_bits(5, OW, mode))
        return ([("a", _image(2, C, 4, 5, fmt), "far")],
                lambda ops, dev: R.resize(ops["a"], (7, OW), mode=mode, weight_bits=wb,
                                          data_format=fmt, nb=1))
    return make


def _dwconv_case(fmt, cross, far):
    def make(odd, bits):
        # inner: C * mult (NHWC) or OW (NCHW).  mult = 2 makes NHWC's inner extent even, so its
        # one-element-per-lane form takes C = 3, mult = 1; NCHW's takes W = 5 (OW = 3)
        C, mult, Wd = ((3, 1, 6) if fmt == "NHWC" else (2, 2, 5)) if odd else (2, 2, 6)
        kx, kw = ("far", "dense") if far == "x" else ("dense", "far")
        xs, ws = _image(2, C, _IMG_H, Wd, fmt), (C * mult, 1, 3, 3)
        specs = [("x0", xs, kx), ("w0", ws, kw)]
        if cross:
            specs += [("x1", xs, kx), ("w1", ws, kw)]
        kw_ = dict(strides=_WIN["strides"], pads=_WIN["pads"], dilations=_WIN["dilations"],
                   data_format=fmt, nb=1)
        if cross:
            return specs, lambda ops, dev: R.dwconv_cross(ops["x0"], ops["x1"], ops["w0"],
                                                          ops["w1"], **kw_)
        return specs, lambda ops, dev: R.dwconv(ops["x0"], ops["w0"], **kw_)
    return make


def _ints(seed, n, bits):
    gen = torch.Generator().manual_seed(seed)
    return [int.from_bytes(bytes(torch.randint(0, 256, (bits // 8,), generator=gen).tolist()),
                           "little") for _ in range(n)]


def _pwl_case(far):
    def make(odd, bits):  # k = 3, cross; 257 / 258 elements cross a block of 256 lanes
        n, k = (257 if odd else 258), 3
        ks, kx = ("far", "dense") if far == "s" else ("dense", "far")
        specs = [("s0", (k, n), ks), ("s1", (k, n), ks), ("x0", (n,), kx), ("x1", (n,), kx)]
        da, db, ak = _ints(1, k, bits), _ints(2, k, bits), _ints(3, 1, bits)[0]
        return specs, lambda ops, dev: R.pwl_cross(ops["s0"], ops["s1"], ops["x0"], ops["x1"],
                                                   da, db, ak, nb=1)
    return make


def _pwp_case(far):
    def make(odd, bits):  # d = 3, k = 3, cross
        n, k, d = (257 if odd else 258), 3, 3
        # "mixed": every power at a stride of its own -- far, EDGE64 and dense
        kinds = ("far", "dense", "dense", "dense") if far == "s" else \
            ("dense", "far", "edge64", "dense")
        specs = [("s0", (k, n), kinds[0]), ("s1", (k, n), kinds[0])]
        for i in range(d):
            specs += [(f"p0{i}", (n,), kinds[1 + i]), (f"p1{i}", (n,), kinds[1 + i])]
        D = [_ints(10 + i, k, bits) for i in range(d + 1)]
        CK = _ints(20, d, bits)
        return specs, lambda ops, dev: R.pwp_cross(
            ops["s0"], ops["s1"], [ops[f"p0{i}"] for i in range(d)],
            [ops[f"p1{i}"] for i in range(d)], D, CK, nb=1)
    return make


# n = 8; (k, j) = (2, 1), (8, 2), (8, 4) with inner = 1: r = j = 1 takes form 2, an even r form
# 1 (both u64 with aligned operands; u128 and a misaligned u64 take form 0); the last is table
# mode, rows of 3 ordered by column 1
_STAGES = {"k2j1": R.CswapGeom(5, 8, 1, -1, 2, 1, False), "k8j2": R.CswapGeom(5, 8, 1, -1, 8, 2, True),
           "k8j4": R.CswapGeom(5, 8, 1, -1, 8, 4, False), "table": R.CswapGeom(2, 8, 3, 1, 4, 2, True)}


def _cswap_shapes(g):
    return ((g.outer, g.n, g.inner), (g.outer, g.n // 2, g.cols), (g.outer, g.n // 2, g.inner))


def _cswap_diff_case(g):
    def make(odd, bits):
        return [("x", _cswap_shapes(g)[0], "far")], lambda ops, dev: R.cswap_diff(ops["x"], g, nb=1)
    return make


def _cswap_cross_case(g, far):
    def make(odd, bits):
        xs, ss, _ = _cswap_shapes(g)
        kx, ks = ("far", "dense") if far == "x" else ("dense", "far")
        specs = [("s0", ss, ks), ("s1", ss, ks), ("x0", xs, kx), ("x1", xs, kx)]
        return specs, lambda ops, dev: R.cswap_cross(ops["s0"], ops["s1"], ops["x0"], ops["x1"], g,
                                                     nb=1)
    return make


def _cswap_apply_case(g, far):
    def make(odd, bits):
        xs, _, ps = _cswap_shapes(g)
        kx, kp = ("far", "dense") if far == "x" else ("dense", "far")
        return ([("x", xs, kx), ("p", ps, kp)],
                lambda ops, dev: R.cswap_apply(ops["x"], ops["p"], g, nb=1))
    return make


def _perm_gather_case(shape, far):
    def make(odd, bits):  # [outer, n, inner]: inner = 6 can take two u64 per lane, inner = 3 not
        specs = [(name, shape, "far" if name == far else "dense") for name in "abpm"]
        perm = torch.tensor([3, 0, 4, 1, 2], dtype=torch.int64)
        return specs, lambda ops, dev: R.perm_gather(ops["a"], perm.to(dev), ops["b"], ops["p"],
                                                     ops["m"], axis=1, nb=1)
    return make


for _fmt in ("NCHW", "NHWC"):
    _case(f"im2col-{_fmt}", "mx_im2col", HEADROOM_ROWS, _im2col_case(_fmt),
          forms=(U64X2, U64X1, U128, U8))
    _case(f"col2im-{_fmt}", "mx_col2im", HEADROOM_LANES, _col2im_case(_fmt))
    for _mode in ("nearest", "linear"):
        _case(f"resize-{_mode}-{_fmt}", "mx_resize2d", HEADROOM_LANES, _resize_case(_fmt, _mode))
    for _cross in (False, True):
        for _far in ("x", "w"):
            _case(f"dwconv-{'cross' if _cross else 'plain'}-{_fmt}-far_{_far}", "mx_dwconv",
                  HEADROOM_LANES, _dwconv_case(_fmt, _cross, _far))
for _far in ("s", "x"):
    _case(f"pwl_cross-far_{_far}", "mx_pwl_cross", HEADROOM_LANES, _pwl_case(_far))
for _far in ("s", "mixed"):
    _case(f"pwp_cross-far_{_far}", "mx_pwp_cross", HEADROOM_LANES, _pwp_case(_far))
for _name, _g in _STAGES.items():
    _case(f"cswap_diff-{_name}", "mx_cswap_diff", HEADROOM_LANES, _cswap_diff_case(_g))
    for _far in ("x", "s"):
        _case(f"cswap_cross-{_name}-far_{_far}", "mx_cswap_cross", HEADROOM_LANES,
              _cswap_cross_case(_g, _far))
    for _far in ("x", "p"):
        _case(f"cswap_apply-{_name}-far_{_far}", "mx_cswap_apply", HEADROOM_LANES,
              _cswap_apply_case(_g, _far))
for _shape in ((2, 5, 6), (2, 5, 3)):
    for _far in "abpm":
        _case(f"perm_gather-{'x'.join(map(str, _shape))}-far_{_far}", "mx_perm_gather",
              HEADROOM_ROWS, _perm_gather_case(_shape, _far))


@pytest.mark.gpu
@pytest.mark.parametrize("case, form, which", CASES)
def test_leaf_at_the_index_width_switch(far_buffer, monkeypatch, case, form, which):
    _check(far_buffer, monkeypatch, case, form, which)


def test_every_family_and_form_is_covered():
    ids = [p.id for p in CASES]
    assert len(ids) == len(set(ids))
    for family in ("im2col", "col2im", "resize", "dwconv", "pwl_cross", "pwp_cross", "cswap_diff",
                   "cswap_cross", "cswap_apply", "perm_gather"):
        for form in (U64X2, U64X1, U128):
            for which in STRIDES:
                assert any(i.startswith(family) and i.endswith(f"-{form}-{which}") for i in ids)
    assert sum(i.endswith(f"-{U8}-{FAR}") for i in ids) == 2  # im2col's bit tensors
