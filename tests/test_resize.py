"""The resize layer: ``R.resize_tables`` against the ONNX ``Resize`` formulas in rationals,
``R.resize`` / ``mx_resize2d`` (CPU twin and gfx950 kernel) against a stencil over python
integers, linearity on additive shares, the torch composition, slot views, the share-pair path
of the stacked session, and ``pm.resize2d`` on the local runtime against float64 torch and the
integer model, through the serialised forms and a lowered graph."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import moose_amd as pm
from moose_amd.compiler import passes
from moose_amd.computation import utils as serde
from moose_amd.edsl import tracer
from moose_amd.ir.computation import Computation
from moose_amd.ir.computation import ReplicatedPlacement
from moose_amd.ops import native as nat
from moose_amd.ops import ring as R
from moose_amd.protocols import replicated as rep
from moose_amd.runtime.local import LocalMooseRuntime
from moose_amd.runtime.local import to_native
from moose_amd.runtime.prims import PRIMS
from moose_amd.runtime.session import PV
from moose_amd.runtime.session import StackedSession

PLC = ReplicatedPlacement(("a", "b", "c"))
ROLES = ["alice", "bob", "carole"]
ALICE, BOB, CAROLE = (pm.host_placement(n) for n in ROLES)
REP = pm.replicated_placement("rep", players=[ALICE, BOB, CAROLE])
HALF = Fraction(1, 2)
COORDS = ("half_pixel", "pytorch_half_pixel", "align_corners", "asymmetric")
NEAREST = ("round_prefer_floor", "round_prefer_ceil", "floor", "ceil")
AXES = [(1, 4), (4, 1), (5, 8), (8, 5), (7, 7), (4, 8), (3, 12)]
FORMATS = ("NCHW", "NHWC")
BITS = (64, 128)

# (N, C, (H, W), (OH, OW)): C in {1, 3, 4} -- odd and even inner extents, so one u64 per lane
# and two per lane (NHWC) both run; N = 2
GEOMS = [
    (2, 4, (4, 5), (8, 10)),   # upsampling
    (2, 3, (8, 5), (5, 3)),    # downsampling
    (2, 1, (5, 8), (8, 5)),    # mixed: H up, W down
    (2, 3, (1, 1), (4, 3)),    # 1x1 input
    (2, 4, (7, 7), (7, 7)),    # identity
    (2, 3, (3, 4), (12, 8)),
]
# (mode, coordinate_transformation_mode, nearest_mode)
MODES = [("nearest", "half_pixel", "round_prefer_floor"), ("linear", "half_pixel", "floor"),
         ("linear", "align_corners", "floor"), ("nearest", "asymmetric", "ceil")]
# device cases, three slots each.  ROWS: 73,984 output rows > the 65,536-row grid at C = 1: a
# lane's row loop takes a second trip.  C130 / C67: the inner extent exceeds one block (64
# lanes of two u64, or of one).  W130: the same for NCHW, whose inner extent is OW
ROWS = (1, 1, (136, 136), (272, 272))
C130 = (1, 130, (3, 3), (5, 4))
C67 = (1, 67, (3, 3), (5, 4))
W130 = (1, 2, (3, 65), (4, 130))


# -- the ONNX definition, in rationals -----------------------------------------------------------
def _onnx_coord(o, I, O, ctm, scale=None):  # noqa: E741
    s = scale if scale is not None else Fraction(O, I)
    if ctm == "half_pixel":
        return (o + HALF) / s - HALF
    if ctm == "pytorch_half_pixel":
        return (o + HALF) / s - HALF if O > 1 else Fraction(0)
    if ctm == "align_corners":
        return Fraction(0) if O == 1 else Fraction(o * (I - 1), O - 1)
    return o / s


def _onnx_weights(I, O, mode, ctm, nearest_mode, wb, scale=None):  # noqa: E741
    """[O, I] integer weights in units of 2^-wb, straight from the ONNX text: nearest rounds
    the coordinate and clamps the index; linear takes floor(x), x - floor(x) on the image
    padded with its edge values."""
    clamp = lambda i: min(max(i, 0), I - 1)  # noqa: E731
    out = np.zeros((O, I), dtype=object)
    for o in range(O):
        x = _onnx_coord(o, I, O, ctm, scale)
        if mode == "nearest":
            i = {"floor": math.floor(x), "ceil": math.ceil(x),
                 "round_prefer_floor": math.ceil(x - HALF),
                 "round_prefer_ceil": math.floor(x + HALF)}[nearest_mode]
            out[o, clamp(i)] += 1
        else:
            lo = math.floor(x)
            r = math.floor((x - lo) * (1 << wb) + HALF)
            out[o, clamp(lo)] += (1 << wb) - r
            out[o, clamp(lo + 1)] += r
    return out


def _table_weights(tab, I, wb):  # noqa: E741
    out = np.zeros((tab.shape[1], I), dtype=object)
    for o, (i0, i1, w1) in enumerate(tab.T.tolist()):
        out[o, i0] += (1 << wb) - w1
        out[o, i1] += w1
    return out


@pytest.mark.parametrize("ctm", COORDS)
@pytest.mark.parametrize("axis", AXES, ids=[f"{i}to{o}" for i, o in AXES])
def test_tables_equal_the_onnx_formulas(axis, ctm):
    I, O = axis  # noqa: E741
    for nearest_mode in NEAREST:
        tab = R.resize_tables(I, O, "nearest", ctm, nearest_mode, None, 7)
        assert tab.dtype == np.int32 and tab.shape == (3, O) and not tab[2].any()
        assert (_table_weights(tab, I, 0) == _onnx_weights(I, O, "nearest", ctm, nearest_mode,
                                                           0)).all()
    for wb in (0, 1, 2, 5, 12):
        tab = R.resize_tables(I, O, "linear", ctm, "floor", None, wb)
        assert tab.dtype == np.int32 and tab.shape == (3, O)
        assert (tab[0] >= 0).all() and (tab[0] < I).all()
        assert (tab[1] == np.minimum(tab[0] + 1, I - 1)).all()
        assert (tab[2] >= 0).all() and (tab[2] <= (1 << wb)).all()
        assert wb or not tab[2].any()  # a table of width 0 is a gather
        assert (_table_weights(tab, I, wb) == _onnx_weights(I, O, "linear", ctm, "floor",
                                                            wb)).all()


def test_tables_with_a_given_scale():
    """A given scale is used as its exact binary value, whatever O is: float32 0.3 lies above
    3/10, so 3 / 0.3f lies below 10 and its floor is 9."""
    s = float(np.float32(0.3))
    tab = R.resize_tables(20, 6, "linear", "asymmetric", "floor", s, 12)
    want = _onnx_weights(20, 6, "linear", "asymmetric", "floor", 12, Fraction(s))
    assert (_table_weights(tab, 20, 12) == want).all()
    near = R.resize_tables(20, 6, "nearest", "asymmetric", "floor", s)
    assert near[0].tolist() == [0, 3, 6, 9, 13, 16]
    assert R.resize_tables(20, 6, "nearest", "asymmetric", "floor",
                           Fraction(3, 10))[0].tolist() == [0, 3, 6, 10, 13, 16]
    assert R.resize_scale(2.5) == Fraction(5, 2) and R.resize_scale((5, 2)) == Fraction(5, 2)


def test_identity_and_the_exact_weight_bits():
    """The smallest width in 0..12 at which every weight of the axis is exact, else 12.  5 -> 8
    is exact in 4 bits with half-pixel centres (t in sixteenths) and inexact with aligned
    corners (t in sevenths): that one takes the 12."""
    for ctm in COORDS:
        tab = R.resize_tables(7, 7, "linear", ctm, "floor", None, 0)
        assert (tab[0] == np.arange(7)).all() and not tab[2].any()
        assert R.resize_weight_bits(7, 7, "linear", ctm) == 0
    assert R.resize_weight_bits(4, 8, "linear", "half_pixel") == 2
    assert R.resize_weight_bits(3, 6, "linear", "pytorch_half_pixel") == 2
    assert R.resize_weight_bits(4, 8, "nearest", "asymmetric") == 0
    assert R.resize_weight_bits(5, 8, "linear", "align_corners") == 12
    assert R.resize_weight_bits(8, 5, "linear", "half_pixel") == 12
    assert R.resize_weight_bits(5, 8, "linear", "half_pixel") == 4
    assert R.resize_weight_bits(3, 5, "linear", "align_corners") == 1


# -- the ring stencil ----------------------------------------------------------------------------
def _shape(case, fmt, out=False):
    n, c, hw, ohw = case
    h, w = ohw if out else hw
    return (n, c, h, w) if fmt == "NCHW" else (n, h, w, c)


def _attrs(case, mode):
    _n, _c, (h, w), (oh, ow) = case
    m, ctm, nm = mode
    wb = (R.resize_weight_bits(h, oh, m, ctm, nm), R.resize_weight_bits(w, ow, m, ctm, nm))
    return dict(sizes=(oh, ow), mode=m, coordinate_transformation_mode=ctm, nearest_mode=nm,
                scales=(), weight_bits=wb)


def _rand_ints(shape, bits, seed):
    """Top bit set everywhere (the high words travel, the sums wrap), and the edge values 0,
    2^k - 1 and 2^(k - 1) in the first places."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    top = 1 << (bits - 1)
    vals = [top | int.from_bytes(rng.bytes(bits // 8), "little") for _ in range(n)]
    vals[:3] = [0, (1 << bits) - 1, top][:n]
    return np.array(vals, dtype=object).reshape(shape)


def _reference(x, case, fmt, attrs, bits=None):
    """Resize of an object array of python ints by explicit loops over the four taps; mod
    2^bits, or exact (signed inputs) when bits is None."""
    n, c, (h, w), (oh, ow) = case
    m, ctm, nm = attrs["mode"], attrs["coordinate_transformation_mode"], attrs["nearest_mode"]
    wbh, wbw = (0, 0) if m == "nearest" else attrs["weight_bits"]
    th = R.resize_tables(h, oh, m, ctm, nm, None, wbh).tolist()
    tw = R.resize_tables(w, ow, m, ctm, nm, None, wbw).tolist()
    xn = x if fmt == "NHWC" else x.transpose(0, 2, 3, 1)
    out = np.zeros((n, oh, ow, c), dtype=object)
    for oy in range(oh):
        ys = ((th[0][oy], (1 << wbh) - th[2][oy]), (th[1][oy], th[2][oy]))
        for ox in range(ow):
            xs = ((tw[0][ox], (1 << wbw) - tw[2][ox]), (tw[1][ox], tw[2][ox]))
            for iy, wy in ys:
                for ix, wx in xs:
                    out[:, oy, ox, :] += xn[:, iy, ix, :] * (wy * wx)
    if bits is not None:
        out = out & ((1 << bits) - 1)
    return out if fmt == "NHWC" else out.transpose(0, 3, 1, 2)


def _ints(rt):
    return np.asarray(R.to_ints(R.RT(rt.data.cpu(), rt.bits)), dtype=object)


_CPU = {}


def _cpu_result(case, fmt, bits, mode, slots=0):
    """(input, CPU twin's output) of a case, computed once and shared."""
    key = (case, fmt, bits, mode, slots)
    if key not in _CPU:
        shape = ((slots,) if slots else ()) + _shape(case, fmt)
        if int(np.prod(shape)) > 4096:  # random words, top bit set
            g = torch.Generator().manual_seed(7)
            x = R.RT(torch.randint(-2**63, 0, shape + ((2,) if bits == 128 else ()),
                                   generator=g, dtype=torch.int64), bits)
        else:
            x = R.from_ints(_rand_ints(shape, bits, 11), bits, "cpu")
        _CPU[key] = (x, R.resize(x, **_attrs(case, mode), data_format=fmt,
                                 nb=1 if slots else 0))
    return _CPU[key]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("mode", MODES, ids=[f"{m[0]}-{m[1]}" for m in MODES])
@pytest.mark.parametrize("case", GEOMS, ids=range(len(GEOMS)))
def test_cpu_twin_equals_python_integers(case, mode, bits, fmt):
    x, got = _cpu_result(case, fmt, bits, mode)
    want = _reference(_ints(x), case, fmt, _attrs(case, mode), bits)
    assert got.shape == want.shape == _shape(case, fmt, out=True)
    assert (_ints(got) == want).all()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("bits", BITS)
def test_linear_on_additive_shares(bits, fmt):
    case, mode = GEOMS[0], MODES[2]  # 12-bit weights on both axes
    attrs = _attrs(case, mode)
    assert attrs["weight_bits"] == (12, 12)
    mask = (1 << bits) - 1
    shares = [_rand_ints(_shape(case, fmt), bits, s) for s in (1, 2, 3)]
    secret = (shares[0] + shares[1] + shares[2]) & mask
    outs = [_ints(R.resize(R.from_ints(s, bits, "cpu"), **attrs, data_format=fmt))
            for s in shares]
    assert (((outs[0] + outs[1] + outs[2]) & mask) == _reference(secret, case, fmt, attrs,
                                                                  bits)).all()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("mode", MODES[:3], ids=[f"{m[0]}-{m[1]}" for m in MODES[:3]])
@pytest.mark.parametrize("case", GEOMS, ids=range(len(GEOMS)))
def test_cpu_twin_equals_the_torch_composition(case, mode, bits, fmt):
    x, want = _cpu_result(case, fmt, bits, mode)
    a = _attrs(case, mode)
    geom = R.resize_geometry(x.shape, a["sizes"], a["mode"], a["coordinate_transformation_mode"],
                             a["nearest_mode"], (), a["weight_bits"], fmt)
    got = R.resize_torch(x.data, geom, a["mode"], a["coordinate_transformation_mode"],
                         a["nearest_mode"], fmt, 0, bits)
    assert got.is_contiguous() and torch.equal(got, want.data)


def test_float_and_bit_tensors_take_the_torch_path():
    case, mode = GEOMS[0], MODES[1]
    a = _attrs(case, mode)
    x = torch.tensor(np.random.default_rng(3).uniform(-1, 1, _shape(case, "NCHW")))
    got = PRIMS["Resize"].impl(0, x, **a, data_format="NCHW")
    want = F.interpolate(x, size=case[3], mode="bilinear", align_corners=False)
    assert got.dtype == torch.float64 and torch.allclose(got, want, rtol=0, atol=1e-15)
    near = _attrs(case, ("nearest", "asymmetric", "floor"))
    bits = R.RT((x > 0).to(torch.uint8), 1)
    for v in (R.resize(bits, **near, data_format="NCHW").data,
              PRIMS["Resize"].impl(0, x > 0, **near, data_format="NCHW").to(torch.uint8)):
        assert torch.equal(v, F.interpolate(bits.data.double(), size=case[3],
                                            mode="nearest").to(torch.uint8))
    with pytest.raises(ValueError, match="linear"):
        R.resize(bits, **a, data_format="NCHW")
    with pytest.raises(ValueError, match="linear"):
        PRIMS["Resize"].impl(0, x > 0, **a, data_format="NCHW")


def test_native_entry_rejects_one_byte_elements_and_bad_tables():
    a = torch.zeros(9, dtype=torch.uint8)
    out = torch.zeros(36, dtype=torch.uint8)
    tab = torch.zeros((3, 6), dtype=torch.int32)
    call = lambda eb, src, dst, t, wb: nat.lib().mx_resize2d(  # noqa: E731
        0, eb, nat.ptr(src), nat.ptr(dst), 1, 9, 1, 1, 3, 3, 6, 6, nat.ptr(t), nat.ptr(t), wb,
        wb, 0, None)
    assert call(1, a, out, tab, 0) == -2
    x, y = torch.zeros(9, dtype=torch.int64), torch.zeros(36, dtype=torch.int64)
    assert call(8, x, y, tab, 0) == 0
    assert call(8, x, y, tab, 13) == -3
    bad = tab.clone()
    bad[1, 2] = 3  # an index outside the 3-pixel axis
    assert call(8, x, y, bad, 2) == -3
    bad = tab.clone()
    bad[2, 0] = 5  # a weight above 2^2
    assert call(8, x, y, bad, 2) == -3


def test_bad_arguments_are_named():
    z = R.zeros((1, 2, 3, 3), 64, "cpu")
    assert R.resize(z, (6, 6)).shape == (1, 2, 6, 6)
    with pytest.raises(ValueError, match="rank-4"):
        R.resize(R.zeros((2, 3, 3), 64, "cpu"), (6, 6))
    with pytest.raises(ValueError, match="sizes"):
        R.resize(z, (6, 0))
    with pytest.raises(ValueError, match="sizes"):
        R.resize(z, (6,))
    with pytest.raises(ValueError, match="`mode`"):
        R.resize(z, (6, 6), mode="cubic")
    with pytest.raises(ValueError, match="coordinate_transformation_mode"):
        R.resize(z, (6, 6), coordinate_transformation_mode="tf_crop_and_resize")
    with pytest.raises(ValueError, match="nearest_mode"):
        R.resize(z, (6, 6), nearest_mode="round")
    with pytest.raises(ValueError, match="weight_bits"):
        R.resize(z, (6, 6), mode="linear", weight_bits=(13, 0))
    with pytest.raises(ValueError, match="data_format"):
        R.resize(z, (6, 6), data_format="CHWN")
    with pytest.raises(ValueError, match="scales"):
        R.resize(z, (6, 6), scales=(2.0,))


def test_meta_tensors_answer_the_shape_only():
    case = GEOMS[1]
    for fmt in FORMATS:
        m = R.RT(torch.empty(_shape(case, fmt), dtype=torch.int64, device="meta"), 64)
        out = R.resize(m, **_attrs(case, MODES[1]), data_format=fmt)
        assert out.device.type == "meta" and out.shape == _shape(case, fmt, out=True)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("bits", BITS)
def test_batch_axis_and_slot_views(bits, fmt):
    case, mode = GEOMS[0], MODES[1]
    a = dict(_attrs(case, mode), data_format=fmt)
    buf, got = _cpu_result(case, fmt, bits, mode, slots=4)
    for s in range(4):  # nb=1 over a 4-slot buffer: four separate calls
        assert torch.equal(got.data[s], R.resize(R.RT(buf.data[s], bits), **a).data)
    view = R.RT(buf.data[1:4], bits)  # a slot view that does not start at the storage
    assert torch.equal(R.resize(view, **a, nb=1).data, got.data[1:4])
    # in_slot_stride larger than the dense size: every second slot, read in place
    strided = R.RT(buf.data[::2], bits)
    assert not strided.data.is_contiguous()
    assert torch.equal(R.resize(strided, **a, nb=1).data, got.data[::2])


def _pair_path(device):
    """A replicated value whose share vectors are the two views of one ring4 buffer goes
    through rep.local as ONE launch over the buffer's four slots; the result is again one
    buffer, equal to the two separate calls and to the CPU twin."""
    case, fmt, mode = GEOMS[0], "NHWC", MODES[1]
    a = dict(_attrs(case, mode), data_format=fmt)
    for bits in BITS:
        sess = StackedSession(device, seed=5)
        shape = _shape(case, fmt)
        s0, s1 = R.ring4((3,) + shape, bits, device)
        src = R.from_ints(_rand_ints((4,) + shape, bits, 9), bits, device)
        s0.data.copy_(src.data[0:3])
        s1.data[2].copy_(src.data[3])
        assert s1.data.data_ptr() == s0.data.data_ptr() + s0.data[0].numel() * 8
        x = rep.RepTensor(PLC, bits, "arith", PV(PLC, s0), PV(PLC, s1))
        y = rep.local(sess, x, "Resize", **a)
        o0, o1 = y.s0.v, y.s1.v
        assert o0.shape == (3,) + _shape(case, fmt, out=True)
        assert o1.data.data_ptr() == o0.data.data_ptr() + o0.data[0].numel() * 8
        assert o0.data.untyped_storage().data_ptr() == o1.data.untyped_storage().data_ptr()
        assert torch.equal(o0.data, R.resize(s0, **a, nb=1).data)
        assert torch.equal(o1.data, R.resize(s1, **a, nb=1).data)
        want = R.resize(R.RT(src.data.cpu(), bits), **a, nb=1)
        assert torch.equal(o0.data.cpu(), want.data[0:3])
        assert torch.equal(o1.data.cpu(), want.data[1:4])


def test_pair_path_cpu():
    _pair_path("cpu")


# -- pm.resize2d on the runtime --------------------------------------------------------------------
DTYPES = {"fixed24_40": (pm.fixed(24, 40), 40, 128), "fixed14_23": (pm.fixed(14, 23, ring=64),
                                                                    23, 64)}
# (name, input (N, C, H, W), sizes, resize2d keywords, F.interpolate keywords).  The ratios are
# powers of two, so torch's float coordinate is the rational one (checked below).  `coarse`
# overrides the weight widths: 1 bit on H is inexact (t in quarters), 2 bits on W exact
E2E = [
    ("bilinear", (2, 3, 4, 5), (8, 10), dict(mode="linear"),
     dict(mode="bilinear", align_corners=False)),
    ("aligned", (2, 3, 3, 5), (5, 9),
     dict(mode="linear", coordinate_transformation_mode="align_corners"),
     dict(mode="bilinear", align_corners=True)),
    ("nearest", (2, 3, 4, 5), (8, 10),
     dict(mode="nearest", coordinate_transformation_mode="asymmetric", nearest_mode="floor"),
     dict(mode="nearest")),
    ("coarse", (2, 3, 4, 5), (8, 10), dict(mode="linear", weight_bits=(1, 2)),
     dict(mode="bilinear", align_corners=False)),
]


def _program(shape, sizes, dt, fmt="NCHW", **kw):
    arg = (None,) + tuple(shape[1:])

    @pm.computation
    def resize(x: pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64), shape=arg)):
        with ALICE:
            xf = pm.cast(x, dtype=dt)
        with REP:
            y = pm.resize2d(xf, sizes=sizes, data_format=fmt, **kw)
        with CAROLE:
            return pm.cast(y, dtype=pm.float64)

    return resize


def _torch_coords_agree(I, O, kw):  # noqa: E741
    """torch's float source coordinate of every output index equals the rational one."""
    for o in range(O):
        if kw["mode"] == "nearest":
            got, want = math.floor(o * (I / O)), math.floor(Fraction(o * I, O))
        elif kw["align_corners"]:
            got, want = ((I - 1) / (O - 1)) * o, Fraction(o * (I - 1), O - 1)
        else:
            got = max((o + 0.5) * (I / O) - 0.5, 0.0)
            want = max((o + HALF) * Fraction(I, O) - HALF, 0)
        if Fraction(got) != want:
            return False
    return True


def _e2e(device, case, dtype, graphs=False):
    name, shape, sizes, kw, tkw = case
    dt, f, ring = DTYPES[dtype]
    for I, O in zip(shape[2:], sizes):  # noqa: E741
        assert _torch_coords_agree(I, O, tkw)
    # multiples of 2^-10 in [-3, 3]: the encoding is exact whatever way it rounds
    x = np.random.default_rng(5).integers(-3072, 3073, shape) / 1024.0
    want = F.interpolate(torch.tensor(x), size=sizes, **tkw).numpy()
    ctm, nm = kw.get("coordinate_transformation_mode", "half_pixel"), kw.get(
        "nearest_mode", "round_prefer_floor")
    exact = tuple(R.resize_weight_bits(i, o, kw["mode"], ctm, nm)
                  for i, o in zip(shape[2:], sizes))
    wb = kw.get("weight_bits", exact)
    assert wb == {"bilinear": (2, 2), "aligned": (1, 1), "nearest": (0, 0),
                  "coarse": (1, 2)}[name]
    attrs = dict(mode=kw["mode"], coordinate_transformation_mode=ctm, nearest_mode=nm,
                 weight_bits=wb)
    xi = np.array([int(v) for v in (x * 1024).reshape(-1)], dtype=object).reshape(shape)
    xi = xi * (1 << (f - 10))
    m = 0 if kw["mode"] == "nearest" else sum(wb)
    model = _reference(xi, (shape[0], shape[1], shape[2:], sizes), "NCHW", attrs)
    model = np.vectorize(lambda v: v >> m, otypes=[object])(model)  # arithmetic shift
    # input encoding + truncation + the weights' rounding on each inexact axis
    bound = 2.0 ** -(f + 1) + 2 * 2.0 ** -f + sum(
        np.abs(x).max() * 2.0 ** (1 - b) for b, e in zip(wb, exact) if b < e)
    gkw = {"use_graphs": True} if graphs else {}
    rt = LocalMooseRuntime(ROLES, device=device, fixedpoint_ring=ring, **gkw)
    comp = _program(shape, sizes, dt, **kw)
    outs = [rt.evaluate_computation(comp, {"x": x})["output_0"] for _ in range(2)]
    for got in outs:  # with hipGraphs on a device the second evaluation is a replay
        assert got.shape == want.shape
        ints = np.rint(got * 2.0 ** f)
        ulp = np.abs(ints - model.astype(np.float64)).max()
        err = np.abs(got - want).max()
        print(f"resize2d {name} {dtype} on {device}: {ulp:.0f} ulp of the integer model, err "
              f"{err:.3e} bound {bound:.3e}")
        assert ulp <= 1 and err <= bound
    assert np.abs(outs[0] - outs[1]).max() <= 2.0 ** -f


@pytest.mark.parametrize("case", E2E, ids=[c[0] for c in E2E])
def test_resize2d_fixed24_40_cpu(case):
    _e2e("cpu", case, "fixed24_40")


def test_resize2d_fixed14_23_ring64_cpu():
    _e2e("cpu", E2E[0], "fixed14_23")


def test_resize2d_nhwc_scales_and_host_placements():
    """NHWC with scales on the replicated placement, and the host paths: fixed point (Sar)
    and float64 on a host agree with torch."""
    x = np.random.default_rng(8).integers(-3072, 3073, (2, 4, 5, 3)) / 1024.0
    want = F.interpolate(torch.tensor(x).permute(0, 3, 1, 2), size=(8, 10), mode="bilinear",
                         align_corners=False).permute(0, 2, 3, 1).numpy()
    dt = pm.fixed(24, 40)

    @pm.computation
    def prog(x: pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64),
                            shape=(None, 4, 5, 3))):
        with ALICE:
            xf = pm.cast(x, dtype=dt)
            hf = pm.cast(pm.resize2d(xf, scales=(2.0, 2.0), mode="linear",
                                     data_format="NHWC"), dtype=pm.float64)
            hd = pm.resize2d(x, scales=(2.0, 2.0), mode="linear", data_format="NHWC")
        with REP:
            y = pm.resize2d(xf, scales=(2.0, 2.0), mode="linear", data_format="NHWC")
            assert y.static_shape == (None, 8, 10, 3)
        with CAROLE:
            return pm.cast(y, dtype=pm.float64), hf, hd

    out = LocalMooseRuntime(ROLES, device="cpu").evaluate_computation(prog, {"x": x})
    bound = 2.0 ** -41 + 2 * 2.0 ** -40
    for k in sorted(out):
        assert out[k].shape == want.shape and np.abs(out[k] - want).max() <= bound


def test_edsl_argument_errors_and_static_shape():
    with ALICE:
        x = pm.constant(np.zeros((1, 2, 4, 4)))
        with pytest.raises(ValueError, match="`sizes` and `scales`"):
            pm.resize2d(x)
        with pytest.raises(ValueError, match="`sizes` and `scales`"):
            pm.resize2d(x, sizes=(8, 8), scales=(2.0, 2.0))
        with pytest.raises(ValueError, match="rank-4"):
            pm.resize2d(pm.constant(np.zeros((2, 4, 4))), sizes=(8, 8))
        with pytest.raises(ValueError, match="`sizes` must be positive"):
            pm.resize2d(x, sizes=(8, 0))
        with pytest.raises(ValueError, match="`scales`"):
            pm.resize2d(x, scales=(2.0, -1.0))
        with pytest.raises(ValueError, match="`scales`.*no output"):
            pm.resize2d(x, scales=(0.1, 1.0))
        with pytest.raises(ValueError, match="`mode`"):
            pm.resize2d(x, sizes=(8, 8), mode="cubic")
        with pytest.raises(ValueError, match="coordinate_transformation_mode"):
            pm.resize2d(x, sizes=(8, 8), coordinate_transformation_mode="tf_crop_and_resize")
        with pytest.raises(ValueError, match="nearest_mode"):
            pm.resize2d(x, sizes=(8, 8), nearest_mode="round")
        with pytest.raises(ValueError, match="data_format"):
            pm.resize2d(x, sizes=(8, 8), data_format="CHWN")
        with pytest.raises(ValueError, match="weight_bits"):
            pm.resize2d(x, sizes=(8, 8), mode="linear", weight_bits=(13, 1))
        with pytest.raises(ValueError, match="linear.*bool"):
            pm.resize2d(pm.constant(np.zeros((1, 2, 4, 4), dtype=np.bool_)), sizes=(8, 8),
                        mode="linear")
        # 24 + 36 + 24 = 84 > 62: the truncation in Z_2^64 has no headroom
        tight = pm.cast(x, dtype=pm.fixed(24, 36, ring=64))
        with pytest.raises(ValueError, match="smaller `weight_bits`"):
            pm.resize2d(tight, sizes=(8, 8), mode="linear", weight_bits=(12, 12))
        # and the exact 2 + 2 bits of a 2x resize fit six bits lower
        fits = pm.cast(x, dtype=pm.fixed(24, 30, ring=64))
        assert pm.resize2d(fits, sizes=(8, 8), mode="linear").static_shape == (1, 2, 8, 8)
        with pytest.raises(ValueError, match="smaller `weight_bits`"):
            pm.resize2d(fits, sizes=(8, 8), mode="linear", weight_bits=(12, 12))
        assert pm.resize2d(x, scales=(1.5, 2.6)).static_shape == (1, 2, 6, 10)
    arg = pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64), shape=(None, 4, 4, 2))

    @pm.computation
    def free(x: arg):
        with ALICE:
            y = pm.resize2d(x, sizes=(3, 9), data_format="NHWC")
            assert y.static_shape == (None, 3, 9, 2)
            with pytest.raises(ValueError, match="batch size"):
                pm.resize2d(x, sizes=(3, 9), input_shape=(None, None, 4, 2))
        return y

    tracer.trace(free)


# -- structure -------------------------------------------------------------------------------------
def _structural():
    shape = (2, 3, 4, 5)
    x = np.random.default_rng(7).integers(-3072, 3073, shape) / 1024.0
    return _program(shape, (8, 10), pm.fixed(24, 40), mode="linear"), {"x": x}


def test_serialised_forms_round_trip_and_evaluate_equal():
    comp, args = _structural()
    native = to_native(comp)
    ops = [op for op in native.operations if op.kind == "Resize"]
    assert len(ops) == 1
    assert {k: (list(v) if isinstance(v, (list, tuple)) else v)
            for k, v in ops[0].attrs.items()} == {
        "sizes": [8, 10], "mode": "linear", "coordinate_transformation_mode": "half_pixel",
        "nearest_mode": "round_prefer_floor", "scales": [], "weight_bits": [2, 2],
        "data_format": "NCHW"}
    txt = native.to_textual()
    assert "Resize{" in txt and 'mode = "linear"' in txt and "weight_bits = [2, 2]" in txt
    from_txt = Computation.from_textual(txt)
    from_mp = Computation.from_msgpack(native.to_msgpack())
    assert from_txt.to_textual() == txt and from_mp.to_textual() == txt
    want = LocalMooseRuntime(ROLES, device="cpu", seed=3).evaluate_computation(comp, args)
    for c in (from_txt, from_mp):
        got = LocalMooseRuntime(ROLES, device="cpu", seed=3).evaluate_compiled(c, args)
        assert all(np.array_equal(got[k], want[k]) for k in want)
    traced = tracer.trace(comp)
    back = serde.deserialize_computation(serde.serialize_computation(traced))
    ro = [op for op in back.operations.values() if type(op).__name__ == "ResizeOperation"]
    assert ro and list(ro[0].sizes) == [8, 10] and ro[0].mode == "linear"
    assert list(ro[0].weight_bits) == [2, 2] and list(ro[0].scales) == []
    # given scales travel as exact ratios
    with ALICE:
        e = pm.resize2d(pm.constant(np.zeros((1, 1, 4, 4))), scales=(2.5, 0.75))
    assert e.attrs["scales"] == [5, 2, 3, 4] and e.attrs["sizes"] == [10, 3]


def test_lowered_graph_has_resize_host_ops_and_agrees():
    comp, args = _structural()
    stacked = LocalMooseRuntime(ROLES, device="cpu", seed=7).evaluate_computation(comp, args)
    low = passes.compile(to_native(comp), arg_specs={"x": args["x"].shape})
    assert passes.is_lowered(low)
    passes.well_formed(low)
    resizes = [op for op in low.operations if op.kind == "Resize"]
    assert resizes and all(type(op.placement).__name__ == "HostPlacement" for op in resizes)
    out = LocalMooseRuntime(ROLES, device="cpu", seed=7).evaluate_compiled(
        Computation.from_textual(low.to_textual()), args)
    # the lowered graph draws its own TruncPr masks: one unit of 2^-40 either way
    for k in stacked:
        assert out[k].shape == stacked[k].shape
        assert np.abs(out[k] - stacked[k]).max() <= 2.0 ** -40


_TYPING = """
x = Constant{{value = HostFloat64Tensor({x})}}: () -> Tensor<Float64> () @Host(alice)
y = Resize{{sizes = [4, 6], mode = "{mode}", coordinate_transformation_mode = "asymmetric", nearest_mode = "floor", scales = [], weight_bits = [{wb}, 1], data_format = "NCHW"}}: (Tensor<Float64>) -> Tensor<Float64> (x) @Host(alice)
out = Output{{tag = "output_0"}}: (Tensor<Float64>) -> Tensor<Float64> (y) @Host(alice)
"""


def test_static_shape_pass_types_and_rejects():
    x = np.arange(12.0).reshape(1, 2, 2, 3)
    good = _TYPING.format(x=x.tolist(), mode="nearest", wb=1)
    passes.typing_pass(Computation.from_textual(good))
    out = LocalMooseRuntime(ROLES, device="cpu").evaluate_compiled(
        Computation.from_textual(good), {})["output_0"]
    assert np.array_equal(out, np.repeat(np.repeat(x, 2, axis=2), 2, axis=3))
    with pytest.raises(passes.CompilationError, match="rank-4"):
        passes.typing_pass(Computation.from_textual(
            _TYPING.format(x=np.zeros((2, 2, 3)).tolist(), mode="nearest", wb=1)))
    with pytest.raises(passes.CompilationError, match="`mode`"):
        passes.typing_pass(Computation.from_textual(
            _TYPING.format(x=x.tolist(), mode="cubic", wb=1)))
    with pytest.raises(passes.CompilationError, match="weight_bits"):
        passes.typing_pass(Computation.from_textual(
            _TYPING.format(x=x.tolist(), mode="linear", wb=13)))


# -- gfx950 ----------------------------------------------------------------------------------------
GPU_MODES = [MODES[0], MODES[1]]  # nearest: the one-load path; linear: four taps


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("mode", GPU_MODES, ids=["nearest", "linear"])
@pytest.mark.parametrize("case", GEOMS + [C130, C67, W130],
                         ids=list(range(len(GEOMS))) + ["c130", "c67", "w130"])
def test_kernel_equals_cpu_twin(case, mode, bits, fmt):
    slots = 3 if case in (C130, C67, W130) else 0
    x, want = _cpu_result(case, fmt, bits, mode, slots)
    got = R.resize(R.RT(x.data.cuda(), bits), **_attrs(case, mode), data_format=fmt,
                   nb=1 if slots else 0)
    assert got.data.is_cuda and torch.equal(got.data.cpu(), want.data)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("mode", GPU_MODES + [MODES[2]], ids=["nearest", "linear", "aligned"])
def test_kernel_row_loop(mode, bits):
    """NHWC [1, 136, 136, 1] -> 272 x 272: 73,984 rows, so the row grid-stride loop takes a
    second trip.  Only the 32-bit index forms run here: the 64-bit ones run in
    test_leaf_index_forms.py, on slots 2^31 elements apart."""
    x, want = _cpu_result(ROWS, "NHWC", bits, mode)
    assert want.shape[1] * want.shape[2] > 65536
    got = R.resize(R.RT(x.data.cuda(), bits), **_attrs(ROWS, mode), data_format="NHWC")
    assert torch.equal(got.data.cpu(), want.data)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_kernel_reads_slot_views_in_place(fmt):
    case, mode = GEOMS[0], MODES[1]
    a = dict(_attrs(case, mode), data_format=fmt)
    for bits in BITS:
        x, want = _cpu_result(case, fmt, bits, mode, slots=4)
        buf = x.data.cuda()
        got = R.resize(R.RT(buf[1:4], bits), **a, nb=1)
        assert torch.equal(got.data.cpu(), want.data[1:4])
        got = R.resize(R.RT(buf[::2], bits), **a, nb=1)
        assert torch.equal(got.data.cpu(), want.data[::2])


@pytest.mark.gpu
def test_kernel_equals_the_torch_composition_on_the_device():
    """The A/B baseline computes what the kernel computes, Z_2^128's limb sums included."""
    case, mode = GEOMS[0], MODES[2]
    for bits in BITS:
        for fmt in FORMATS:
            x, want = _cpu_result(case, fmt, bits, mode, slots=4)
            a = dict(_attrs(case, mode), data_format=fmt)
            xd = R.RT(x.data.cuda(), bits)
            R.RESIZE_KERNEL = False
            try:
                got = R.resize(xd, **a, nb=1)
            finally:
                R.RESIZE_KERNEL = True
            assert got.data.is_cuda and torch.equal(got.data.cpu(), want.data)


@pytest.mark.gpu
def test_pair_path_gpu():
    _pair_path("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_resize2d_bilinear_gpu(dtype):
    _e2e("cuda:0", E2E[0], dtype, graphs=True)
