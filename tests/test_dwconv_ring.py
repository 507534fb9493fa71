"""The depthwise-convolution ring layer: ``R.dwconv`` / ``R.dwconv_cross`` / ``mx_dwconv`` (CPU
twin and gfx950 kernel ``k_dwconv``) against explicit python loops over python integers.
Exact equality only: operands are uniform over the whole ring, so every sum wraps.  Every case
runs on the host and, marked ``gpu``, on the device; the integer model is computed once per
case and shared."""
import numpy as np
import pytest
import torch

from moose_amd.ops import ring as R

DEVICES = ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)]
FORMATS = ("NCHW", "NHWC")
BITS = (64, 128)
MODES = ("plain", "cross")

# (N, C, H, W), mult, kernel, strides, pads (top, left, bottom, right), dilations
ASYM1 = ((2, 3, 5, 4), 1, (3, 2), (2, 1), (1, 0, 2, 1), (1, 2))  # odd channels: the u64 tail
ASYM2 = ((2, 3, 5, 4), 2, (3, 2), (2, 1), (1, 0, 2, 1), (1, 2))  # two outputs per channel
ONES = ((1, 1, 3, 3), 1, (3, 3), (1, 1), (1, 1, 1, 1), (1, 1))
# 130 channels: a third block of 64 u128 lanes (a second of 128 u64) along the channels
CHANNELS = ((1, 130, 3, 3), 1, (3, 3), (1, 1), (1, 1, 1, 1), (1, 1))
# past the row grid of 65,536 rows, so a lane's row loop takes a second trip: NHWC rows are
# (n, oh, ow) = 67,600; NCHW rows are (n, oh) = 65,540
TALL = {"NHWC": ((1, 1, 260, 260), 1, (1, 1), (1, 1), (0, 0, 0, 0), (1, 1)),
        "NCHW": ((1, 1, 65540, 1), 1, (1, 1), (1, 1), (0, 0, 0, 0), (1, 1))}


def _x_shape(case, fmt):
    n, c, h, w = case[0]
    return (n, c, h, w) if fmt == "NCHW" else (n, h, w, c)


def _w_shape(case):
    return (case[0][1] * case[1], 1) + tuple(case[2])


def _rand_ints(shape, bits, seed):
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    vals = [int.from_bytes(rng.bytes(bits // 8), "little") for _ in range(n)]
    return np.array(vals, dtype=object).reshape(shape)


def _reference(x0, x1, w0, w1, case, fmt, bits):
    """sum_taps x0 (w0 + w1) + x1 w0 mod 2^bits (x1 is None: sum_taps x0 w0), on object arrays
    of python ints, by explicit loops."""
    (N, C, H, W), mult, (KH, KW), (sh, sw), (pt, pl, pb, pr), (dh, dw) = case
    mask = (1 << bits) - 1
    OH = (H + pt + pb - dh * (KH - 1) - 1) // sh + 1
    OW = (W + pl + pr - dw * (KW - 1) - 1) // sw + 1
    nchw = fmt == "NCHW"
    at = (lambda a, n, c, y, z: a[n, c, y, z]) if nchw else (lambda a, n, c, y, z: a[n, y, z, c])
    out = np.zeros((N, C * mult, OH, OW) if nchw else (N, OH, OW, C * mult), dtype=object)
    for n in range(N):
        for oc in range(C * mult):
            c = oc // mult
            for oh in range(OH):
                for ow in range(OW):
                    acc = 0
                    for kh in range(KH):
                        for kw in range(KW):
                            y, z = oh * sh + kh * dh - pt, ow * sw + kw * dw - pl
                            if not (0 <= y < H and 0 <= z < W):
                                continue
                            a, b = at(x0, n, c, y, z), w0[oc, 0, kh, kw]
                            if x1 is None:
                                acc += a * b
                            else:
                                acc += a * (b + w1[oc, 0, kh, kw]) + at(x1, n, c, y, z) * b
                    if nchw:
                        out[n, oc, oh, ow] = acc & mask
                    else:
                        out[n, oh, ow, oc] = acc & mask
    return out


def _ints(rt):
    return np.asarray(R.to_ints(R.RT(rt.data.cpu(), rt.bits)), dtype=object)


_MODEL = {}


def _model(name, case, fmt, bits, mode, ones=False):
    """(operands as object arrays, expected output) of a case, computed once."""
    key = (name, fmt, bits, mode)
    if key not in _MODEL:
        xs, ws = _x_shape(case, fmt), _w_shape(case)
        if ones:
            top = (1 << bits) - 1
            ops = [np.full(s, top, dtype=object) for s in (xs, xs, ws, ws)]
        else:
            ops = [_rand_ints(s, bits, 20 + i) for i, s in enumerate((xs, xs, ws, ws))]
        x0, x1, w0, w1 = ops
        if mode == "plain":
            x1 = w1 = None
        _MODEL[key] = ((x0, x1, w0, w1), _reference(x0, x1, w0, w1, case, fmt, bits))
    return _MODEL[key]


def _run(ops, case, fmt, bits, device):
    x0, x1, w0, w1 = (None if a is None else R.from_ints(a, bits, device) for a in ops)
    attrs = (case[3], case[4], case[5], fmt)
    if x1 is None:
        return R.dwconv(x0, w0, *attrs)
    return R.dwconv_cross(x0, x1, w0, w1, *attrs)


def _check(name, case, fmt, bits, mode, device, ones=False):
    ops, want = _model(name, case, fmt, bits, mode, ones)
    got = _run(ops, case, fmt, bits, device)
    assert got.device.type == device.split(":")[0]
    assert tuple(got.shape) == want.shape
    assert (_ints(got) == want).all()


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ("asym1", "asym2"))
def test_asymmetric_geometry(name, mode, bits, fmt, device):
    _check(name, {"asym1": ASYM1, "asym2": ASYM2}[name], fmt, bits, mode, device)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("mode", MODES)
def test_all_ones_carries_and_padded_corners(mode, bits, fmt, device):
    _check("ones", ONES, fmt, bits, mode, device, ones=True)
    _, want = _model("ones", ONES, fmt, bits, mode, True)
    # (2^b - 1)^2 = 1 mod 2^b: a corner sums 4 taps, the centre 9 (three times that in cross)
    k = 3 if mode == "cross" else 1
    flat = want.reshape(3, 3)
    assert flat[0, 0] == 4 * k and flat[1, 1] == 9 * k


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("mode", MODES)
def test_more_than_one_block_of_channels(mode, bits, fmt, device):
    _check("channels", CHANNELS, fmt, bits, mode, device)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("mode", MODES)
def test_past_the_row_grid(mode, bits, fmt, device):
    """1x1 kernel, one channel: out = x0 (w0 + w1) + x1 w0 elementwise (one weight), on more
    rows than the row grid holds."""
    case = TALL[fmt]
    key = ("tall", fmt, bits, mode)
    if key not in _MODEL:
        xs = _x_shape(case, fmt)
        mask = (1 << bits) - 1
        x0, x1 = _rand_ints(xs, bits, 31), _rand_ints(xs, bits, 32)
        w0, w1 = _rand_ints((1, 1, 1, 1), bits, 33), _rand_ints((1, 1, 1, 1), bits, 34)
        a, b = int(w0.reshape(-1)[0]), int(w1.reshape(-1)[0])
        if mode == "plain":
            _MODEL[key] = ((x0, None, w0, None), (x0 * a) & mask)
        else:
            _MODEL[key] = ((x0, x1, w0, w1), (x0 * (a + b) + x1 * a) & mask)
    ops, want = _MODEL[key]
    assert want.size > 65536
    got = _run(ops, case, fmt, bits, device)
    assert tuple(got.shape) == want.shape and (_ints(got) == want).all()


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("bits", BITS)
def test_operand_views(bits, fmt, device):
    """Operands that are the two views of a four-slot share-pair buffer (s0 = buf[0:3], s1 =
    buf[1:4]) and every second slot of it (a slot stride that is not dense) are read in place;
    a rank-4 weight or image beside batched operands is public (slot stride 0)."""
    case = ASYM2
    xs, ws = _x_shape(case, fmt), _w_shape(case)
    attrs = (case[3], case[4], case[5], fmt)
    key = ("views", fmt, bits)
    if key not in _MODEL:
        xb, wb = _rand_ints((4,) + xs, bits, 41), _rand_ints((4,) + ws, bits, 42)
        cross = [_reference(xb[s], xb[s + 1], wb[s], wb[s + 1], case, fmt, bits) for s in range(3)]
        plain = [_reference(xb[s], None, wb[s], None, case, fmt, bits) for s in range(4)]
        pubw = [_reference(xb[s], None, wb[1], None, case, fmt, bits) for s in range(4)]
        pubx = [_reference(xb[2], None, wb[s], None, case, fmt, bits) for s in range(4)]
        pubw_cross = [_reference(xb[s], xb[s + 1], wb[0], wb[3], case, fmt, bits)
                      for s in range(3)]
        _MODEL[key] = (xb, wb, cross, plain, pubw, pubx, pubw_cross)
    xb, wb, cross, plain, pubw, pubx, pubw_cross = _MODEL[key]
    X, Wt = R.from_ints(xb, bits, device), R.from_ints(wb, bits, device)
    rt = lambda d: R.RT(d, bits)  # noqa: E731

    def same(got, want):
        return (_ints(got) == np.stack(want)).all()

    # the share-pair views
    got = R.dwconv_cross(rt(X.data[0:3]), rt(X.data[1:4]), rt(Wt.data[0:3]), rt(Wt.data[1:4]),
                         *attrs, nb=1)
    assert same(got, cross)
    # all four slots in one launch, and a slot stride of two slots
    assert same(R.dwconv(X, Wt, *attrs, nb=1), plain)
    strided = rt(X.data[::2])
    assert not strided.data.is_contiguous()
    assert same(R.dwconv(strided, rt(Wt.data[::2]), *attrs, nb=1), plain[::2])
    # public weight, public image
    assert same(R.dwconv(X, rt(Wt.data[1]), *attrs, nb=1), pubw)
    assert same(R.dwconv(rt(X.data[2]), Wt, *attrs, nb=1), pubx)
    assert same(R.dwconv_cross(rt(X.data[0:3]), rt(X.data[1:4]), rt(Wt.data[0]), rt(Wt.data[3]),
                               *attrs, nb=1), pubw_cross)


def test_geometry():
    g = R.dwconv_geometry((2, 3, 5, 4), (6, 1, 3, 2), (2, 1), (1, 0, 2, 1), (1, 2), "NCHW")
    assert g == (2, 3, 5, 4, 2, 3, 2, 2, 1, 1, 0, 2, 1, 1, 2, 3, 3)
    assert R.dwconv_geometry((2, 5, 4, 3), (3, 1, 1, 1), data_format="NHWC")[4] == 1
    with pytest.raises(ValueError, match=r"w.shape\[1\] = 3"):
        R.dwconv_geometry((1, 3, 4, 4), (3, 3, 1, 1))
    with pytest.raises(ValueError, match="multiple of the input's 3 channels"):
        R.dwconv_geometry((1, 3, 4, 4), (4, 1, 1, 1))
    with pytest.raises(ValueError, match="rank-4"):
        R.dwconv_geometry((3, 4, 4), (3, 1, 1, 1))
    with pytest.raises(ValueError, match="rank-4 weight"):
        R.dwconv_geometry((1, 3, 4, 4), (3, 1, 1))
    with pytest.raises(ValueError, match="dwconv.*does not fit"):
        R.dwconv_geometry((1, 3, 2, 2), (3, 1, 3, 3))


def test_meta_and_bits():
    x = R.RT(torch.empty((3, 2, 5, 4, 3), dtype=torch.int64, device="meta"), 64)
    w = R.RT(torch.empty((3, 6, 1, 3, 2), dtype=torch.int64, device="meta"), 64)
    out = R.dwconv_cross(x, x, w, w, (2, 1), (1, 0, 2, 1), (1, 2), "NHWC", nb=1)
    assert tuple(out.shape) == (3, 2, 3, 3, 6) and out.device.type == "meta"
    bit = R.RT(torch.zeros((1, 1, 2, 2), dtype=torch.uint8), 1)
    with pytest.raises(ValueError, match="arithmetic only"):
        R.dwconv(bit, R.RT(torch.zeros((1, 1, 1, 1), dtype=torch.uint8), 1))
