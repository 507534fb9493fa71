"""pm.conv_transpose2d / pm.col2im against float64 torch on every runtime, and the Col2Im
operator through typing, lowering and the serialised forms."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import moose_amd as pm
from moose_amd.compiler import passes
from moose_amd.computation import utils as serde
from moose_amd.edsl import tracer
from moose_amd.ir.computation import Computation
from moose_amd.runtime.local import LocalMooseRuntime
from moose_amd.runtime.local import to_native

ROLES = ["alice", "bob", "carole"]
ALICE, BOB, CAROLE = (pm.host_placement(n) for n in ROLES)
REP = pm.replicated_placement("rep", players=[ALICE, BOB, CAROLE])
MIR = pm.mirrored_placement("mir", players=[ALICE, BOB, CAROLE])
# tests/test_col2im.py's geometries read as transposed convolutions: the image (N, OC, OHt,
# OWt) is the OUTPUT, x is [N, C', OH, OW]: image, kernel, strides, pads, dilations, (OH, OW),
# C', output_padding
GEOMS = [
    ((2, 2, 5, 3), (3, 2), (2, 1), (1, 0, 2, 1), (1, 2), (3, 2), 3, (1, 0)),
    ((1, 3, 7, 9), (2, 2), (3, 3), (0, 0, 0, 0), (1, 1), (2, 3), 2, (2, 1)),
    ((1, 2, 3, 3), (3, 3), (1, 1), (1, 1, 1, 1), (1, 1), (3, 3), 1, (0, 0)),
    ((2, 5, 6, 6), (1, 1), (2, 2), (0, 0, 0, 0), (1, 1), (3, 3), 4, (1, 1)),
    ((1, 2, 11, 6), (2, 3), (3, 2), (0, 2, 1, 0), (2, 1), (4, 3), 2, (0, 1)),
    ((1, 1, 3, 3), (3, 3), (1, 1), (0, 0, 0, 0), (1, 1), (1, 1), 1, (0, 0)),
]
DTYPES = {64: pm.fixed(14, 23), 128: pm.fixed(24, 40)}
FRAC = {64: 23, 128: 40}


def _grid(a, f):
    """The fixed-point grid value the encoder gives (it truncates)."""
    return np.trunc(a * 2.0 ** f) / 2.0 ** f


def _nhwc(a):
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))


def _x_shape(geom, fmt):
    n, (oh, ow), c = geom[0][0], geom[5], geom[6]
    return (n, c, oh, ow) if fmt == "NCHW" else (n, oh, ow, c)


def _torch_reference(x, w, bias, geom):
    """F.conv_transpose2d without padding, zero-padded by output_padding at the bottom and
    the right, cropped by the pads; the bias reaches every pixel."""
    (_n, _oc, ht, wt), _k, strides, (pt, pl, _pb, _pr), dil, _o, _c, (oph, opw) = geom
    full = F.conv_transpose2d(x, w, None, stride=strides, padding=0, dilation=dil)
    full = F.pad(full, (0, opw, 0, oph))
    out = full[:, :, pt:pt + ht, pl:pl + wt]
    assert out.shape[2:] == (ht, wt)
    return out if bias is None else out + bias.reshape(1, -1, 1, 1)


def _multiplicity(geom):
    """The most patch-matrix entries any output pixel sums."""
    (oh, ow), kernel = geom[5], geom[1]
    ones = _torch_reference(torch.ones(1, 1, oh, ow, dtype=torch.float64),
                            torch.ones((1, 1) + kernel, dtype=torch.float64), None, geom)
    return int(ones.max())


def _program(geom, fmt, ring, mirrored, w, b, outputs=(0, 1)):
    _img, _kernel, strides, pads, dil, _ohw, _c, opad = geom
    dt = DTYPES[ring]

    @pm.computation
    def convt(x: pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64),
                             shape=_x_shape(geom, fmt))):
        with ALICE:
            xf = pm.cast(x, dtype=dt)
        with (MIR if mirrored else BOB):
            wf = pm.cast(pm.constant(w), dtype=dt)
            bf = pm.cast(pm.constant(b), dtype=dt)
        with REP:
            ys = [pm.conv_transpose2d(xf, wf, bf if i else None, strides=strides, pads=pads,
                                      dilations=dil, output_padding=opad, data_format=fmt)
                  for i in outputs]
        with CAROLE:
            return tuple(pm.cast(y, dtype=pm.float64) for y in ys)

    return convt


def _runtime(device, ring, **kw):
    if device != "cpu":
        kw.setdefault("use_graphs", True)
    return LocalMooseRuntime(ROLES, device=device, fixedpoint_ring=ring, **kw)


def _twice(rt, comp, args):
    """Two evaluations: with hipGraphs on a device the second one is a replay."""
    first = rt.evaluate_computation(comp, args)
    second = rt.evaluate_computation(comp, args)
    return [[r[k] for k in sorted(r)] for r in (first, second)]


def _inputs(geom, seed=5):
    (n, oc, _h, _w), kernel, (oh, ow), c = geom[0], geom[1], geom[5], geom[6]
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (n, c, oh, ow)), rng.uniform(-1, 1, (c, oc) + kernel),
            rng.uniform(-1, 1, (oc,)))


def _check(device, gi, fmt, ring, mirrored):
    geom = GEOMS[gi]
    f = FRAC[ring]
    x, w, b = _inputs(geom)
    xt, wt, bt = (torch.tensor(_grid(v, f)) for v in (x, w, b))
    refs = [_torch_reference(xt, wt, bias, geom).numpy() for bias in (None, bt)]
    # A patch-matrix entry is a dot of C' products, exact in the ring at 2f fractional bits;
    # bounding each product by one unit of 2^-f (had it been truncated on its own) and adding
    # TruncPr's own probabilistic unit gives C' + 1 units per entry.  A pixel sums at most T
    # entries (the largest multiplicity of this geometry, exactly, in the ring), and the bias
    # adds one unit: (T * (C' + 1) + 1) * 2^-f.  The float64 reference is exact far below that.
    T, c = _multiplicity(geom), geom[6]
    tol = (T * (c + 1) + 1) * 2.0 ** -f
    comp = _program(geom, fmt, ring, mirrored, w, b)
    arg = x if fmt == "NCHW" else _nhwc(x)
    for outs in _twice(_runtime(device, ring), comp, {"x": arg}):
        for got, ref in zip(outs, refs):
            want = ref if fmt == "NCHW" else _nhwc(ref)
            assert got.shape == want.shape
            err = np.abs(got - want).max()
            print(f"conv_transpose2d G{gi} {fmt} ring{ring} mirrored={mirrored} T={T}: "
                  f"err {err:.3e} tol {tol:.3e}")
            assert err <= tol


CASES = [(g, fmt, ring, mir) for g in range(len(GEOMS)) for fmt in ("NCHW", "NHWC")
         for ring in (64, 128) for mir in (False, True)]
# on the device: every geometry in both layouts, the (ring, weight) pairs taking turns so
# that each layout sees all four
GPU_CASES = [(g, fmt, (64, 128)[(g + i) % 2], bool((g // 2 + i) % 2))
             for g in range(len(GEOMS)) for i, fmt in enumerate(("NCHW", "NHWC"))]


@pytest.mark.parametrize("gi,fmt,ring,mirrored", CASES)
def test_conv_transpose2d_cpu(gi, fmt, ring, mirrored):
    _check("cpu", gi, fmt, ring, mirrored)


@pytest.mark.gpu
@pytest.mark.parametrize("gi,fmt,ring,mirrored", GPU_CASES)
def test_conv_transpose2d_gpu(gi, fmt, ring, mirrored):
    _check("cuda:0", gi, fmt, ring, mirrored)


def test_output_geometry_is_the_forward_geometry():
    """The forward geometry of the output image with the same attributes is the input's
    spatial size: output_padding < strides is absorbed by the floor."""
    from moose_amd.ops import ring as R

    for geom in GEOMS:
        img, kernel, strides, pads, dil, ohw, _c, opad = geom
        g = R.im2col_geometry(img, kernel, strides, pads, dil)
        assert g[-2:] == ohw
        ht = (ohw[0] - 1) * strides[0] + dil[0] * (kernel[0] - 1) + 1 - pads[0] - pads[2] + opad[0]
        wt = (ohw[1] - 1) * strides[1] + dil[1] * (kernel[1] - 1) + 1 - pads[1] - pads[3] + opad[1]
        assert (ht, wt) == img[2:]


# -- structure ----------------------------------------------------------------------------------
def _structural(fmt="NCHW", outputs=(1,)):
    geom = GEOMS[0]
    x, w, b = _inputs(geom, seed=7)
    return (_program(geom, fmt, 128, False, w, b, outputs=outputs),
            {"x": x if fmt == "NCHW" else _nhwc(x)})


def test_stacked_and_per_party_threads_reveal_equal_outputs():
    """A seeded stacked session and the parties as threads reveal the same bits for a program
    with one transposed convolution: Col2Im is applied share-wise by the same primitive."""
    for fmt in ("NCHW", "NHWC"):
        comp, args = _structural(fmt)
        stacked = LocalMooseRuntime(ROLES, device="cpu", seed=7).evaluate_computation(comp, args)
        threads = LocalMooseRuntime(ROLES, device_map={r: "cpu" for r in ROLES},
                                    seed=7).evaluate_computation(comp, args)
        assert sorted(stacked) == sorted(threads)
        for k in stacked:
            assert np.array_equal(stacked[k], threads[k])


def test_lowered_graph_runs_and_agrees():
    comp, args = _structural()
    stacked = LocalMooseRuntime(ROLES, device="cpu", seed=7).evaluate_computation(comp, args)
    low = passes.compile(to_native(comp), arg_specs={"x": args["x"].shape})
    assert passes.is_lowered(low)
    passes.well_formed(low)
    kinds = {op.kind for op in low.operations}
    assert {"Col2Im", "Permute"} <= kinds
    # The lowered graph draws its PRF keys when it runs, so its TruncPr masks are not the
    # stacked session's.  TruncPr reveals floor(q) or floor(q) + 1 units of 2^-40 of each
    # patch-matrix entry's exact q, so two runs differ by at most one unit per entry, and a
    # pixel sums at most T entries (exactly): within T units of each other.
    T = _multiplicity(GEOMS[0])
    out = LocalMooseRuntime(ROLES, device="cpu", seed=7).evaluate_compiled(
        Computation.from_textual(low.to_textual()), args)
    for k in stacked:
        assert out[k].shape == stacked[k].shape
        assert np.abs(out[k] - stacked[k]).max() <= T * 2.0 ** -40


def test_serialised_forms_round_trip():
    comp, _ = _structural()
    native = to_native(comp)
    col = [op for op in native.operations if op.kind == "Col2Im"]
    assert len(col) == 1
    assert {k: (list(v) if isinstance(v, (list, tuple)) else v)
            for k, v in col[0].attrs.items()} == {
        "image_shape": [2, 5, 3], "kernel_shape": [3, 2], "strides": [2, 1],
        "pads": [1, 0, 2, 1], "dilations": [1, 2], "data_format": "NCHW"}
    txt = native.to_textual()
    assert "Col2Im{" in txt and "image_shape = [2, 5, 3]" in txt
    assert Computation.from_textual(txt).to_textual() == txt
    assert Computation.from_msgpack(native.to_msgpack()).to_textual() == txt
    traced = tracer.trace(comp)
    back = serde.deserialize_computation(serde.serialize_computation(traced))
    ci = [op for op in back.operations.values() if type(op).__name__ == "Col2ImOperation"]
    assert ci and list(ci[0].image_shape) == [2, 5, 3] and list(ci[0].kernel_shape) == [3, 2]
    assert list(ci[0].strides) == [2, 1] and list(ci[0].pads) == [1, 0, 2, 1]
    assert list(ci[0].dilations) == [1, 2] and ci[0].data_format == "NCHW"


_TYPING = """
x = Constant{{value = HostFloat64Tensor({x})}}: () -> Tensor<Float64> () @Host(alice)
w = Constant{{value = HostFloat64Tensor({w})}}: () -> Tensor<Float64> () @Host(alice)
c = Dot: (Tensor<Float64>, Tensor<Float64>) -> Tensor<Float64> (x, w) @Host(alice)
y = Col2Im{{image_shape = [2, 3, 3], kernel_shape = [2, 2], strides = [1, 1], pads = [0, 0, 0, 0], dilations = [1, 1], data_format = "NCHW"}}: (Tensor<Float64>) -> Tensor<Float64> (c) @Host(alice)
out = Output{{tag = "output_0"}}: (Tensor<Float64>) -> Tensor<Float64> (y) @Host(alice)
"""


def test_typing_rejects_bad_rank_and_channel_mismatch():
    # a 2x2 input of 3 channels, w = [3, OC*KH*KW = 8]: every pixel of the 3x3 output sums
    # its 1, 2 or 4 taps of 3.0
    good = _TYPING.format(x=np.ones((4, 3)).tolist(), w=np.ones((3, 8)).tolist())
    passes.typing_pass(Computation.from_textual(good))
    out = LocalMooseRuntime(ROLES, device="cpu").evaluate_compiled(
        Computation.from_textual(good), {})["output_0"]
    mult = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], dtype=np.float64)
    assert np.array_equal(out, np.broadcast_to(3.0 * mult, (1, 2, 3, 3)))
    # the weight gives 9 columns: not the 8 of 2 output channels under a 2x2 kernel
    channels = _TYPING.format(x=np.ones((4, 3)).tolist(), w=np.ones((3, 9)).tolist())
    with pytest.raises(passes.CompilationError, match="columns"):
        passes.typing_pass(Computation.from_textual(channels))
    # the input's channels do not match the weight's
    inner = _TYPING.format(x=np.ones((4, 2)).tolist(), w=np.ones((3, 8)).tolist())
    with pytest.raises(passes.CompilationError, match="channels"):
        passes.typing_pass(Computation.from_textual(inner))
    rows = _TYPING.format(x=np.ones((5, 3)).tolist(), w=np.ones((3, 8)).tolist())
    with pytest.raises(passes.CompilationError, match="multiple"):
        passes.typing_pass(Computation.from_textual(rows))
    rank3 = _TYPING.replace("c = Dot: (Tensor<Float64>, Tensor<Float64>) -> Tensor<Float64> "
                            "(x, w)", "c = Identity: (Tensor<Float64>) -> Tensor<Float64> (x)")
    rank3 = rank3.format(x=np.ones((1, 4, 8)).tolist(), w=np.ones((3, 8)).tolist())
    with pytest.raises(passes.CompilationError, match="rank-2"):
        passes.typing_pass(Computation.from_textual(rank3))


def test_edsl_argument_errors():
    with ALICE:
        x = pm.constant(np.zeros((1, 2, 3, 3)))
        w = pm.constant(np.zeros((2, 4, 3, 3)))
        with pytest.raises(ValueError, match="output_padding"):
            pm.conv_transpose2d(x, w, strides=(2, 2), output_padding=(2, 0))
        with pytest.raises(ValueError, match="output_padding"):
            pm.conv_transpose2d(x, w, output_padding=(0, 1))
        with pytest.raises(ValueError, match="output_padding"):
            pm.conv_transpose2d(x, w, strides=(2, 2), output_padding=(0, -1))
        with pytest.raises(ValueError, match="output_padding"):
            pm.conv_transpose2d(x, w, strides=(2, 2), output_padding=(1,))
        with pytest.raises(ValueError, match="channels"):
            pm.conv_transpose2d(x, pm.constant(np.zeros((3, 4, 3, 3))))
        with pytest.raises(ValueError, match="C, OC, KH, KW"):
            pm.conv_transpose2d(x, pm.constant(np.zeros((2, 4, 3))))
        with pytest.raises(ValueError, match="rank-4"):
            pm.conv_transpose2d(pm.constant(np.zeros((2, 3, 3))), w)
        with pytest.raises(ValueError, match="no output"):
            pm.conv_transpose2d(x, pm.constant(np.zeros((2, 4, 1, 1))), pads=(2, 0, 1, 0))
        with pytest.raises(ValueError, match="data_format"):
            pm.conv_transpose2d(x, w, data_format="CHWN")
        with pytest.raises(ValueError, match="positive"):
            pm.conv_transpose2d(x, w, strides=(0, 1))
        fx = pm.cast(x, dtype=pm.fixed(14, 23))
        fw = pm.cast(w, dtype=pm.fixed(14, 23))
        y = pm.conv_transpose2d(fx, fw, strides=(2, 2), pads=(1, 1, 1, 1), output_padding=(1, 1))
        assert y.static_shape == (1, 4, 6, 6)
        # col2im on its own: the result carries the image, the batch comes from the rows
        cols = pm.constant(np.zeros((18, 8)))
        assert pm.col2im(cols, (2, 4, 4), (2, 2)).static_shape == (2, 2, 4, 4)
        assert pm.col2im(cols, (2, 4, 4), (2, 2), data_format="NHWC").static_shape == (2, 4, 4, 2)
        with pytest.raises(ValueError, match="patch matrix"):
            pm.col2im(cols, (3, 4, 4), (2, 2))
        with pytest.raises(ValueError, match="multiple"):
            pm.col2im(pm.constant(np.zeros((10, 8))), (2, 4, 4), (2, 2))
        with pytest.raises(ValueError, match="does not fit"):
            pm.col2im(cols, (2, 1, 1), (2, 2))
        with pytest.raises(ValueError, match="image_shape"):
            pm.col2im(cols, (2, 4), (2, 2))

    @pm.computation
    def shapeless(x: pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64))):
        with ALICE:
            return pm.conv_transpose2d(x, pm.constant(np.zeros((2, 4, 3, 3))))

    with pytest.raises(ValueError, match="static shape"):
        tracer.trace(shapeless)
