"""The col2im ring layer: ``R.col2im`` / ``mx_col2im`` (CPU twin and gfx950 kernel), the exact
adjoint of im2col, against a reference of explicit python loops over python integers; the
adjoint identities; linearity on additive shares; the torch path of plain tensors against
``F.fold`` + crop; slot views and the share-pair path of the stacked session."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from moose_amd.ir.computation import ReplicatedPlacement
from moose_amd.ops import ring as R
from moose_amd.protocols import replicated as rep
from moose_amd.runtime.prims import PRIMS
from moose_amd.runtime.session import PV
from moose_amd.runtime.session import StackedSession

PLC = ReplicatedPlacement(("a", "b", "c"))

# image (N, C, H, W), kernel, strides, pads (top, left, bottom, right), dilations, (OH, OW)
GEOMS = [
    # overlap, asymmetric pads, dilation
    ((2, 2, 5, 3), (3, 2), (2, 1), (1, 0, 2, 1), (1, 2), (3, 2)),
    # stride > kernel: pixels without a contribution, trailing rows / columns no window reaches
    ((1, 3, 7, 9), (2, 2), (3, 3), (0, 0, 0, 0), (1, 1), (2, 3)),
    # 4 to 9 taps per pixel
    ((1, 2, 3, 3), (3, 3), (1, 1), (1, 1, 1, 1), (1, 1), (3, 3)),
    # 1x1 with holes
    ((2, 5, 6, 6), (1, 1), (2, 2), (0, 0, 0, 0), (1, 1), (3, 3)),
    # left pad only, dilated rows
    ((1, 2, 11, 6), (2, 3), (3, 2), (0, 2, 1, 0), (2, 1), (4, 3)),
    # kernel equals image
    ((1, 1, 3, 3), (3, 3), (1, 1), (0, 0, 0, 0), (1, 1), (1, 1)),
]
# three slots each; more than one block in each grid direction.  Inner extent (NHWC: C, NCHW:
# W) 130 is even: u64 takes two per lane (128 per block), 16-byte loads and stores; 67 is
# odd: one u64 per lane (64 per block).  Rows: 25 (NHWC) or 10 (NCHW) over blocks of 4
LARGE = [
    ((1, 130, 5, 5), (3, 3), (2, 2), (1, 1, 1, 1), (1, 1), (3, 3)),
    ((1, 67, 5, 5), (3, 3), (2, 2), (1, 1, 1, 1), (1, 1), (3, 3)),
    ((1, 2, 5, 130), (3, 3), (2, 2), (1, 1, 1, 1), (1, 1), (3, 65)),
    ((1, 2, 5, 67), (3, 3), (2, 2), (1, 1, 1, 1), (1, 1), (3, 34)),
]
# output rows = 66,000 (NHWC: N*H*W) or 132,000 (NCHW: N*C*H) > 65,536 = the row grid: a
# lane's row loop takes a second trip; two channels, one column and two taps keep it cheap
TALL = ((1, 2, 66000, 1), (2, 1), (1, 1), (1, 0, 0, 0), (1, 1), (66000, 1))
FORMATS = ("NCHW", "NHWC")
BITS = (64, 128)


def _image(case, fmt):
    n, c, h, w = case[0]
    return (n, c, h, w) if fmt == "NCHW" else (n, h, w, c)


def _cols_shape(case):
    (n, c, _h, _w), (kh, kw), (oh, ow) = case[0], case[1], case[5]
    return (n * oh * ow, c * kh * kw)


def _args(case, fmt):
    return (tuple(case[0][1:]),) + tuple(case[1:5]) + (fmt,)


def _rand_ints(shape, bits, seed):
    """Every value has its top bit set: the high words must travel and the sums must wrap."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    top = 1 << (bits - 1)
    vals = [top | int.from_bytes(rng.bytes(bits // 8), "little") for _ in range(n)]
    return np.array(vals, dtype=object).reshape(shape)


def _reference(cols, case, fmt, bits):
    """col2im of an object array of python ints: a scatter by explicit loops, mod 2^bits."""
    (N, C, H, W), (KH, KW), (sh, sw), (pt, pl, _pb, _pr), (dh, dw), (OH, OW) = case
    out = np.zeros(_image(case, fmt), dtype=object)
    for n in range(N):
        for oh in range(OH):
            for ow in range(OW):
                row = (n * OH + oh) * OW + ow
                for c in range(C):
                    for kh in range(KH):
                        for kw in range(KW):
                            y, z = oh * sh + kh * dh - pt, ow * sw + kw * dw - pl
                            col = (c * KH + kh) * KW + kw if fmt == "NCHW" \
                                else (kh * KW + kw) * C + c
                            if 0 <= y < H and 0 <= z < W:
                                idx = (n, c, y, z) if fmt == "NCHW" else (n, y, z, c)
                                out[idx] += cols[row, col]
    return out & ((1 << bits) - 1)


def _ints(rt):
    return np.asarray(R.to_ints(R.RT(rt.data.cpu(), rt.bits)), dtype=object)


_CPU = {}


def _cpu_result(case, fmt, bits, slots=0):
    """(patch matrix, CPU twin's image) of a case, computed once and shared."""
    key = (id(case), fmt, bits, slots)
    if key not in _CPU:
        shape = ((slots,) if slots else ()) + _cols_shape(case)
        if case is TALL:  # random words, top bit set: python integers would take seconds
            g = torch.Generator().manual_seed(7)
            words = torch.randint(-2**63, 0, shape + ((2,) if bits == 128 else ()),
                                  generator=g, dtype=torch.int64)
            cols = R.RT(words, bits)
        else:
            cols = R.from_ints(_rand_ints(shape, bits, 11), bits, "cpu")
        _CPU[key] = (cols, R.col2im(cols, *_args(case, fmt), nb=1 if slots else 0))
    return _CPU[key]


def test_geometry_set_is_what_im2col_gives():
    for case in GEOMS + LARGE + [TALL]:
        for fmt in FORMATS:
            g = R.im2col_geometry(_image(case, fmt), *case[1:5], fmt)
            assert g[-2:] == case[5]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("case", GEOMS, ids=range(len(GEOMS)))
def test_cpu_twin_equals_python_integers(case, bits, fmt):
    cols, got = _cpu_result(case, fmt, bits)
    want = _reference(_ints(cols), case, fmt, bits)
    assert got.shape == want.shape == _image(case, fmt)
    assert (_ints(got) == want).all()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("case", GEOMS, ids=range(len(GEOMS)))
def test_adjoint_of_im2col(case, bits, fmt):
    """<im2col(x), c> == <x, col2im(c)> mod 2^bits, and col2im(im2col(x)) == x * multiplicity
    (the multiplicity: col2im of a matrix of ones)."""
    mask = (1 << bits) - 1
    cols, img = _cpu_result(case, fmt, bits)
    c, ci = _ints(cols), _ints(img)
    x = _rand_ints(_image(case, fmt), bits, 5)
    xr = R.from_ints(x, bits, "cpu")
    xc = R.im2col(xr, *case[1:5], fmt)
    assert int((_ints(xc) * c).sum()) & mask == int((x * ci).sum()) & mask
    ones = R.from_ints(np.ones(_cols_shape(case), dtype=object), bits, "cpu")
    mult = _ints(R.col2im(ones, *_args(case, fmt)))
    assert mult.max() <= case[1][0] * case[1][1]
    back = _ints(R.col2im(xc, *_args(case, fmt)))
    assert (back == (x * mult) & mask).all()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("bits", BITS)
def test_linear_on_additive_shares(bits, fmt):
    case = GEOMS[1]  # has pixels no window reaches
    mask = (1 << bits) - 1
    shares = [_rand_ints(_cols_shape(case), bits, s) for s in (1, 2, 3)]
    secret = (shares[0] + shares[1] + shares[2]) & mask
    outs = [_ints(R.col2im(R.from_ints(s, bits, "cpu"), *_args(case, fmt))) for s in shares]
    want = _reference(secret, case, fmt, bits)
    assert (((outs[0] + outs[1] + outs[2]) & mask) == want).all()
    # a pixel no window reaches is zero in every share's image; here every other pixel has
    # one contribution, which is never zero (top bit set)
    hole = _reference(np.ones(_cols_shape(case), dtype=object), case, fmt, bits) == 0
    assert hole.any() and not hole.all()
    for o in outs:
        assert (o[hole] == 0).all() and (o[~hole] != 0).all()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("case", GEOMS, ids=range(len(GEOMS)))
def test_torch_path_equals_fold_and_crop(case, fmt):
    (n, c, h, w), kernel, strides, (pt, pl, pb, pr), dil, (oh, ow) = case
    cols = torch.tensor(np.random.default_rng(3).uniform(-1, 1, _cols_shape(case)))
    m = cols
    if fmt == "NHWC":  # columns (kh, kw, c) -> (c, kh, kw)
        m = cols.reshape(-1, kernel[0] * kernel[1], c).permute(0, 2, 1).reshape(cols.shape)
    m = m.reshape(n, oh * ow, -1).permute(0, 2, 1)
    want = F.fold(m, (h + pt + pb, w + pl + pr), kernel, dilation=dil, stride=strides)
    want = want[:, :, pt:pt + h, pl:pl + w]
    if fmt == "NHWC":
        want = want.permute(0, 2, 3, 1)
    got = PRIMS["Col2Im"].impl(0, cols, image_shape=(c, h, w), kernel_shape=kernel,
                               strides=strides, pads=(pt, pl, pb, pr), dilations=dil,
                               data_format=fmt)
    assert got.dtype == torch.float64 and got.is_contiguous() and torch.equal(got, want)
    # and it is the ring kernel's arithmetic: small integers agree exactly
    ints = torch.round(cols * 100).to(torch.int64)
    ring = R.col2im(R.RT(ints, 64), *_args(case, fmt))
    host = PRIMS["Col2Im"].impl(0, ints.to(torch.float64), image_shape=(c, h, w),
                                kernel_shape=kernel, strides=strides, pads=(pt, pl, pb, pr),
                                dilations=dil, data_format=fmt)
    assert torch.equal(ring.data.to(torch.float64), host)


def test_bool_and_bit_tensors_raise():
    case = GEOMS[2]
    attrs = dict(image_shape=case[0][1:], kernel_shape=case[1], strides=case[2], pads=case[3],
                 dilations=case[4])
    with pytest.raises(ValueError, match="bool"):
        PRIMS["Col2Im"].impl(0, torch.zeros(_cols_shape(case), dtype=torch.bool), **attrs)
    bits = R.RT(torch.zeros(_cols_shape(case), dtype=torch.uint8), 1)
    with pytest.raises(ValueError, match="arithmetic"):
        R.col2im(bits, *_args(case, "NCHW"))
    with pytest.raises(ValueError, match="arithmetic"):
        PRIMS["Col2Im"].impl(0, bits, **attrs)


def test_native_entry_rejects_one_byte_elements():
    from moose_amd.ops import native as nat

    a = torch.zeros(9, dtype=torch.uint8)
    out = torch.zeros(9, dtype=torch.uint8)
    rc = nat.lib().mx_col2im(0, 1, nat.ptr(a), nat.ptr(out), 1, 9, 1, 1, 3, 3, 3, 3, 1, 1, 0,
                             0, 1, 1, 1, 1, 0, None)
    assert rc == -2


def test_bad_geometries_raise():
    z = lambda r, k: R.zeros((r, k), 64, "cpu")  # noqa: E731
    # G2: (C, H, W) = (2, 3, 3), 3x3, pad 1 -> 9 windows, 18 columns
    args = ((2, 3, 3), (3, 3), (1, 1), (1, 1, 1, 1), (1, 1))
    assert R.col2im(z(18, 18), *args).shape == (2, 2, 3, 3)
    with pytest.raises(ValueError, match="columns"):
        R.col2im(z(9, 17), *args)
    with pytest.raises(ValueError, match="multiple"):
        R.col2im(z(10, 18), *args)
    with pytest.raises(ValueError, match="does not fit"):
        R.col2im(z(1, 18), (2, 2, 2), (3, 3))
    with pytest.raises(ValueError, match="rank-2"):
        R.col2im(R.zeros((1, 9, 18), 64, "cpu"), *args)
    with pytest.raises(ValueError, match="image_shape"):
        R.col2im(z(9, 18), (2, 3), (3, 3))
    with pytest.raises(ValueError):
        R.col2im_geometry((9, 18), (2, 3, 3), (3, 3), (1, 1), (1, 1, 1), (1, 1), "NCHW")
    with pytest.raises(ValueError, match="columns"):
        PRIMS["Col2Im"].impl(0, torch.zeros(9, 17), image_shape=(2, 3, 3), kernel_shape=(3, 3),
                             pads=(1, 1, 1, 1))
    assert R.col2im_geometry((18, 18), *args, "NHWC")[:4] == (2, 2, 3, 3)


def test_meta_tensors_answer_the_shape_only():
    case = GEOMS[0]
    for fmt in FORMATS:
        m = R.RT(torch.empty(_cols_shape(case), dtype=torch.int64, device="meta"), 64)
        out = R.col2im(m, *_args(case, fmt))
        assert out.device.type == "meta" and out.shape == _image(case, fmt)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("bits", BITS)
def test_batch_axis_and_slot_views(bits, fmt):
    case = GEOMS[0]
    buf, got = _cpu_result(case, fmt, bits, slots=4)
    for s in range(4):  # nb=1 over a 4-slot buffer: four separate calls
        one = R.col2im(R.RT(buf.data[s], bits), *_args(case, fmt))
        assert torch.equal(got.data[s], one.data)
    view = R.RT(buf.data[1:4], bits)  # a slot view that does not start at the storage
    assert torch.equal(R.col2im(view, *_args(case, fmt), nb=1).data, got.data[1:4])
    # slots that are not dense: every second one of a 4-slot buffer, read in place
    strided = R.RT(buf.data[::2], bits)
    assert not strided.data.is_contiguous()
    assert torch.equal(R.col2im(strided, *_args(case, fmt), nb=1).data, got.data[::2])


@pytest.mark.parametrize("fmt", FORMATS)
def test_tall_twin_against_torch(fmt):
    """The twin on the row-loop case, in wrapping int64: two taps per pixel, out[y, c] =
    cols[y, (c, tap 1)] + cols[y + 1, (c, tap 0)]."""
    cols, want = _cpu_result(TALL, fmt, 64)
    d = cols.data.reshape(66000, 2, 2)  # NCHW: [row, c, kh]; NHWC: [row, kh, c]
    d = d if fmt == "NCHW" else d.transpose(1, 2)
    out = d[:, :, 1].clone()
    out[:-1] += d[1:, :, 0]
    out = out.transpose(0, 1) if fmt == "NCHW" else out  # NCHW image: [c, y]
    assert torch.equal(want.data.reshape(out.shape), out.contiguous())


def _pair_path(device):
    """A replicated value whose share vectors are the two views of one ring4 buffer goes
    through rep.local as ONE launch over the buffer's four slots; the result is again one
    buffer, equal to the two separate calls."""
    case, fmt = GEOMS[0], "NHWC"
    attrs = dict(image_shape=case[0][1:], kernel_shape=case[1], strides=case[2], pads=case[3],
                 dilations=case[4], data_format=fmt)
    for bits in BITS:
        sess = StackedSession(device, seed=5)
        shape = _cols_shape(case)
        s0, s1 = R.ring4((3,) + shape, bits, device)
        src = R.from_ints(_rand_ints((4,) + shape, bits, 9), bits, device)
        s0.data.copy_(src.data[0:3])
        s1.data[2].copy_(src.data[3])
        assert s1.data.data_ptr() == s0.data.data_ptr() + s0.data[0].numel() * 8
        x = rep.RepTensor(PLC, bits, "arith", PV(PLC, s0), PV(PLC, s1))
        y = rep.local(sess, x, "Col2Im", **attrs)
        o0, o1 = y.s0.v, y.s1.v
        assert o0.shape == (3,) + _image(case, fmt)
        assert o1.data.data_ptr() == o0.data.data_ptr() + o0.data[0].numel() * 8
        assert o0.data.untyped_storage().data_ptr() == o1.data.untyped_storage().data_ptr()
        assert torch.equal(o0.data, R.col2im(s0, *_args(case, fmt), nb=1).data)
        assert torch.equal(o1.data, R.col2im(s1, *_args(case, fmt), nb=1).data)
        want = R.col2im(R.RT(src.data.cpu(), bits), *_args(case, fmt), nb=1)
        assert torch.equal(o0.data.cpu(), want.data[0:3])
        assert torch.equal(o1.data.cpu(), want.data[1:4])


def test_pair_path_cpu():
    _pair_path("cpu")


# -- gfx950 -----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("case", GEOMS + LARGE,
                         ids=list(range(len(GEOMS))) + ["c130", "c67", "w130", "w67"])
def test_kernel_equals_cpu_twin(case, bits, fmt):
    slots = 3 if case in LARGE else 0
    cols, want = _cpu_result(case, fmt, bits, slots)
    got = R.col2im(R.RT(cols.data.cuda(), bits), *_args(case, fmt), nb=1 if slots else 0)
    assert got.data.is_cuda and torch.equal(got.data.cpu(), want.data)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_kernel_reads_slot_views_in_place(fmt):
    case = GEOMS[4]
    for bits in BITS:
        cols, want = _cpu_result(case, fmt, bits, slots=4)
        buf = cols.data.cuda()
        got = R.col2im(R.RT(buf[1:4], bits), *_args(case, fmt), nb=1)
        assert torch.equal(got.data.cpu(), want.data[1:4])
        got = R.col2im(R.RT(buf[::2], bits), *_args(case, fmt), nb=1)
        assert torch.equal(got.data.cpu(), want.data[::2])


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("bits", BITS)
def test_kernel_row_loop(bits, fmt):
    """The row grid-stride loop takes a second trip (TALL).  Only the 32-bit index forms run
    here: the 64-bit ones run in test_leaf_index_forms.py, on slots 2^31 elements apart."""
    cols, want = _cpu_result(TALL, fmt, bits)
    rows = want.data.numel() // (2 if bits == 128 else 1) // (2 if fmt == "NHWC" else 1)
    assert rows > 65536
    got = R.col2im(R.RT(cols.data.cuda(), bits), *_args(TALL, fmt))
    assert torch.equal(got.data.cpu(), want.data)


@pytest.mark.gpu
def test_pair_path_gpu():
    _pair_path("cuda:0")
