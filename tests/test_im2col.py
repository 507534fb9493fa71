"""The im2col ring layer: ``R.im2col`` / ``mx_im2col`` (CPU twin and gfx950 kernel) against a
reference of explicit python loops over python integers, the torch path of plain tensors
against ``torch.nn.functional.unfold``, linearity on additive shares, and the share-pair
path of the stacked session."""
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

# set A: (N, C, H, W), kernel, strides, pads (top, left, bottom, right), dilations -- every
# index path: asymmetric pads with stride and dilation, kernel = image, 1x1, left pad only
SET_A = [
    ((2, 3, 5, 4), (3, 2), (2, 1), (1, 0, 2, 1), (1, 2)),
    ((1, 1, 3, 3), (3, 3), (1, 1), (0, 0, 0, 0), (1, 1)),
    ((2, 5, 4, 4), (1, 1), (1, 1), (0, 0, 0, 0), (1, 1)),
    ((1, 2, 6, 7), (2, 3), (3, 2), (0, 2, 0, 0), (1, 1)),
]
# more than one block in both grid directions; K = 72 (NCHW: two u64 per lane) and K = 81
# (NHWC: odd row length, one u64 per lane)
LARGE = ((4, 8, 9, 9), (3, 3), (1, 1), (1, 1, 1, 1), (1, 1))
# rows = 67,600 > 65,536 = the row grid (16,384 blocks of 4 rows): a lane's row loop takes a
# second trip; K = 1 and 1-byte elements keep it cheap
TALL = ((1, 1, 260, 260), (1, 1), (1, 1), (0, 0, 0, 0), (1, 1))
# K = 144 > 128: more than one block along the columns for two u64 per lane as well
WIDE = ((1, 16, 3, 3), (3, 3), (1, 1), (1, 1, 1, 1), (1, 1))
FORMATS = ("NCHW", "NHWC")
BITS = (64, 128, 1)


def _logical(case, fmt):
    """The case's tensor shape in ``fmt``: set A lists (N, C, H, W); LARGE is used as is in
    both formats (its NHWC reading has C = 9)."""
    shp = case[0]
    if case is LARGE or fmt == "NCHW":
        return shp
    n, c, h, w = shp
    return (n, h, w, c)


def _rand_ints(shape, bits, seed):
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    if bits == 1:
        vals = [int(v) for v in rng.integers(0, 2, n)]
    else:  # every value has its top bit set: the high words must travel too
        top = 1 << (bits - 1)
        vals = [top | int.from_bytes(rng.bytes(bits // 8), "little") for _ in range(n)]
    return np.array(vals, dtype=object).reshape(shape)


def _reference(x, kernel, strides, pads, dil, fmt):
    """im2col of an object array of python ints, by explicit loops."""
    if fmt == "NCHW":
        N, C, H, W = x.shape
        at = lambda n, c, y, z: x[n, c, y, z]  # noqa: E731
    else:
        N, H, W, C = x.shape
        at = lambda n, c, y, z: x[n, y, z, c]  # noqa: E731
    (KH, KW), (sh, sw), (pt, pl, pb, pr), (dh, dw) = kernel, strides, pads, dil
    OH = (H + pt + pb - dh * (KH - 1) - 1) // sh + 1
    OW = (W + pl + pr - dw * (KW - 1) - 1) // sw + 1
    out = np.zeros((N * OH * OW, C * KH * KW), dtype=object)
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
                                out[row, col] = at(n, c, y, z)
    return out


def _ints(rt):
    return np.asarray(R.to_ints(R.RT(rt.data.cpu(), rt.bits)), dtype=object)


_CPU = {}


def _cpu_result(case, fmt, bits, slots=0):
    """(input, CPU twin's output) of a case, computed once and shared."""
    key = (id(case), fmt, bits, slots)
    if key not in _CPU:
        shape = ((slots,) if slots else ()) + _logical(case, fmt)
        x = R.from_ints(_rand_ints(shape, bits, 11), bits, "cpu")
        _CPU[key] = (x, R.im2col(x, *case[1:], fmt, nb=1 if slots else 0))
    return _CPU[key]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("case", SET_A, ids=range(len(SET_A)))
def test_cpu_twin_equals_python_integers(case, bits, fmt):
    x, got = _cpu_result(case, fmt, bits)
    want = _reference(_ints(x), *case[1:], fmt)
    assert got.shape == want.shape
    assert (_ints(got) == want).all()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("case", SET_A, ids=range(len(SET_A)))
def test_shape_formula_matches_torch_conv2d(case, fmt):
    shp, kernel, strides, pads, dil = case
    n, c, h, w = shp
    pt, pl, pb, pr = pads
    ref = F.conv2d(F.pad(torch.zeros(shp), (pl, pr, pt, pb)), torch.zeros((1, c) + kernel),
                   stride=strides, dilation=dil)
    geom = R.im2col_geometry(_logical(case, fmt), kernel, strides, pads, dil, fmt)
    assert geom[-2:] == tuple(ref.shape[2:])
    assert _cpu_result(case, fmt, 64)[1].shape == (n * geom[-2] * geom[-1],
                                                   c * kernel[0] * kernel[1])


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("bits", BITS)
def test_batch_axis_and_slot_views(bits, fmt):
    case = SET_A[0]
    buf, got = _cpu_result(case, fmt, bits, slots=4)
    for s in range(4):  # nb=1 over a 4-slot buffer: four separate calls
        one = R.im2col(R.RT(buf.data[s], bits), *case[1:], fmt)
        assert torch.equal(got.data[s], one.data)
    view = R.RT(buf.data[1:4], bits)  # a slot view that does not start at the storage
    assert torch.equal(R.im2col(view, *case[1:], fmt, nb=1).data, got.data[1:4])
    # slots that are not dense: every second one of a 4-slot buffer, read in place
    strided = R.RT(buf.data[::2], bits)
    assert not strided.data.is_contiguous()
    assert torch.equal(R.im2col(strided, *case[1:], fmt, nb=1).data, got.data[::2])


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("case", SET_A, ids=range(len(SET_A)))
def test_torch_path_equals_unfold(case, fmt):
    shp, kernel, strides, pads, dil = case
    n, c, h, w = shp
    pt, pl, pb, pr = pads
    x = torch.tensor(np.random.default_rng(3).uniform(-1, 1, shp))
    u = F.unfold(F.pad(x, (pl, pr, pt, pb)), kernel, dilation=dil, stride=strides)
    want = u.permute(0, 2, 1).reshape(-1, c * kernel[0] * kernel[1])  # rows (n, l), cols (c, kh, kw)
    arg = x
    if fmt == "NHWC":
        arg = x.permute(0, 2, 3, 1).contiguous()
        want = want.reshape(-1, c, kernel[0] * kernel[1]).permute(0, 2, 1).reshape(want.shape)
    got = PRIMS["Im2Col"].impl(0, arg, kernel_shape=kernel, strides=strides, pads=pads,
                               dilations=dil, data_format=fmt)
    assert got.dtype == torch.float64 and torch.equal(got, want)
    # bool host tensors: padding is False
    b = PRIMS["Im2Col"].impl(0, arg > 0, kernel_shape=kernel, strides=strides, pads=pads,
                             dilations=dil, data_format=fmt)
    assert b.dtype == torch.bool and torch.equal(b, want > 0)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("bits", (64, 128))
def test_linear_on_additive_shares(bits, fmt):
    case = SET_A[0]
    shape = _logical(case, fmt)
    mask = (1 << bits) - 1
    shares = [_rand_ints(shape, bits, s) for s in (1, 2, 3)]
    secret = (shares[0] + shares[1] + shares[2]) & mask
    outs = [_ints(R.im2col(R.from_ints(s, bits, "cpu"), *case[1:], fmt)) for s in shares]
    want = _reference(secret, *case[1:], fmt)
    assert (((outs[0] + outs[1] + outs[2]) & mask) == want).all()
    # where the secret's patch matrix is padding, every share's is zero (no share of the
    # input is zero: all have their top bit set)
    pad = _reference(np.ones(shape, dtype=object), *case[1:], fmt) == 0
    assert pad.any()
    for o in outs:
        assert (o[pad] == 0).all() and (o[~pad] != 0).all()


def test_empty_output_is_rejected():
    x = R.zeros((1, 1, 2, 2), 64, "cpu")
    with pytest.raises(ValueError, match="does not fit"):
        R.im2col(x, (3, 3))
    with pytest.raises(ValueError, match="does not fit"):
        R.im2col(x, (2, 2), dilations=(1, 2))
    with pytest.raises(ValueError, match="rank-4"):
        R.im2col(R.zeros((2, 2, 2), 64, "cpu"), (1, 1))
    with pytest.raises(ValueError):
        PRIMS["Im2Col"].impl(0, torch.zeros(1, 1, 2, 2), kernel_shape=(3, 3))


def _pair_path(device):
    """A replicated value whose share vectors are the two views of one ring4 buffer goes
    through rep.local as ONE launch over the buffer's four slots; the result is again one
    buffer, equal to the two separate calls."""
    case, fmt = SET_A[0], "NHWC"
    attrs = dict(kernel_shape=case[1], strides=case[2], pads=case[3], dilations=case[4],
                 data_format=fmt)
    for bits in (64, 128):
        sess = StackedSession(device, seed=5)
        shape = _logical(case, fmt)
        s0, s1 = R.ring4((3,) + shape, bits, device)
        src = R.from_ints(_rand_ints((4,) + shape, bits, 9), bits, device)
        s0.data.copy_(src.data[0:3])
        s1.data[2].copy_(src.data[3])
        assert s1.data.data_ptr() == s0.data.data_ptr() + s0.data[0].numel() * 8
        x = rep.RepTensor(PLC, bits, "arith", PV(PLC, s0), PV(PLC, s1))
        y = rep.local(sess, x, "Im2Col", **attrs)
        o0, o1 = y.s0.v, y.s1.v
        assert o1.data.data_ptr() == o0.data.data_ptr() + o0.data[0].numel() * 8
        assert o0.data.untyped_storage().data_ptr() == o1.data.untyped_storage().data_ptr()
        assert torch.equal(o0.data, R.im2col(s0, *case[1:], fmt, nb=1).data)
        assert torch.equal(o1.data, R.im2col(s1, *case[1:], fmt, nb=1).data)
        # Permute takes the same path
        z = rep.local(sess, x, "Permute", axes=(0, 3, 1, 2))
        assert z.s1.v.data.data_ptr() == z.s0.v.data.data_ptr() + z.s0.v.data[0].numel() * 8
        assert torch.equal(z.s1.v.data, R.transpose(s1, 1, (0, 3, 1, 2)).data)


def test_pair_path_cpu():
    _pair_path("cpu")


# -- gfx950 -----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("case", SET_A + [LARGE], ids=list(range(len(SET_A))) + ["large"])
def test_kernel_equals_cpu_twin(case, bits, fmt):
    slots = 3 if case is LARGE else 0
    x, want = _cpu_result(case, fmt, bits, slots)
    got = R.im2col(R.RT(x.data.cuda(), bits), *case[1:], fmt, nb=1 if slots else 0)
    assert got.data.is_cuda and torch.equal(got.data.cpu(), want.data)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_kernel_reads_slot_views_in_place(fmt):
    case = SET_A[3]
    for bits in BITS:
        x, want = _cpu_result(case, fmt, bits, slots=4)
        buf = x.data.cuda()
        got = R.im2col(R.RT(buf[1:4], bits), *case[1:], fmt, nb=1)
        assert torch.equal(got.data.cpu(), want.data[1:4])
        got = R.im2col(R.RT(buf[::2], bits), *case[1:], fmt, nb=1)
        assert torch.equal(got.data.cpu(), want.data[::2])


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_kernel_row_loop_and_column_blocks(fmt):
    """The row grid-stride loop (TALL) and a second column block at two u64 per lane (WIDE).
    Only the 32-bit index forms run here: the 64-bit ones run in test_leaf_index_forms.py, on
    slots 2^31 elements apart."""
    x, want = _cpu_result(TALL, fmt, 1)
    assert want.shape[0] > 65536
    # K = 1, 1x1, no padding: the patch matrix is the image
    assert torch.equal(want.data.reshape(-1), x.data.reshape(-1))
    got = R.im2col(R.RT(x.data.cuda(), 1), *TALL[1:], fmt)
    assert torch.equal(got.data.cpu(), want.data)
    for bits in (64, 128):
        x, want = _cpu_result(WIDE, fmt, bits)
        assert want.shape[1] == 144
        assert (_ints(want) == _reference(_ints(x), *WIDE[1:], fmt)).all()
        got = R.im2col(R.RT(x.data.cuda(), bits), *WIDE[1:], fmt)
        assert torch.equal(got.data.cpu(), want.data)


@pytest.mark.gpu
def test_pair_path_gpu():
    _pair_path("cuda:0")
