"""The piecewise-linear activations (pm.piecewise_linear, clip, relu6, leaky_relu, hard_sigmoid,
hard_tanh, thresholded_relu, hard_swish) and pm.tanh on the local runtime against float64
numpy, at the integer level against the operator's own tables, on per-party threads, through
the serialised forms, and their trace-time errors."""
from fractions import Fraction

import numpy as np
import pytest

import moose_amd as pm
from moose_amd.compiler import passes
from moose_amd.edsl import tracer
from moose_amd.ir.computation import Computation
from moose_amd.runtime.local import LocalMooseRuntime
from moose_amd.runtime.local import to_native

ROLES = ["alice", "bob", "carole"]
ALICE, BOB, CAROLE = (pm.host_placement(n) for n in ROLES)
REP = pm.replicated_placement("rep", players=[ALICE, BOB, CAROLE])
DTYPES = {64: pm.fixed(14, 23), 128: pm.fixed(24, 40)}
FRAC = {64: 23, 128: 40}
SHAPE = (2, 3, 5, 4)
FAR = 1000.0
DEVICES = ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)]

# name -> (builder, float64 reference, breakpoints, largest |slope|)
PWL = [-1.0, 2.0], [0.0, 1.0, 0.5], [-1.0, 0.0, 1.0]
CONTINUOUS = {
    "piecewise_linear": (lambda t: pm.piecewise_linear(t, *PWL),
                         lambda v: np.where(v < -1, -1.0, np.where(v < 2, v, 0.5 * v + 1)),
                         (-1.0, 2.0), 1.0),
    "relu_as_pwl": (lambda t: pm.piecewise_linear(t, [0], [0, 1], [0, 0]),
                    lambda v: np.maximum(v, 0), (0.0,), 1.0),
    "clip": (lambda t: pm.clip(t, -2.0, 2.5), lambda v: np.clip(v, -2.0, 2.5), (-2.0, 2.5), 1.0),
    "clip_lo": (lambda t: pm.clip(t, lo=-2.0), lambda v: np.maximum(v, -2.0), (-2.0,), 1.0),
    "clip_hi": (lambda t: pm.clip(t, hi=2.5), lambda v: np.minimum(v, 2.5), (2.5,), 1.0),
    "relu6": (pm.relu6, lambda v: np.clip(v, 0, 6), (0.0, 6.0), 1.0),
    "leaky_relu": (lambda t: pm.leaky_relu(t, 0.1), lambda v: np.where(v >= 0, v, 0.1 * v),
                   (0.0,), 1.0),
    "hard_sigmoid": (lambda t: pm.hard_sigmoid(t, 0.2, 0.5),
                     lambda v: np.clip(0.2 * v + 0.5, 0, 1), (-2.5, 2.5), 0.2),
    "hard_tanh": (pm.hard_tanh, lambda v: np.clip(v, -1, 1), (-1.0, 1.0), 1.0),
    # x * hard_sigmoid(x): outside [-3, 3] the factor is exactly 0 or 1 up to TruncPr's unit,
    # which x scales; inside, |x| <= 3 scales the factor's few units.  Lipschitz constant 1.5
    "hard_swish": (pm.hard_swish, lambda v: v * np.clip(v / 6 + 0.5, 0, 1), (-3.0, 3.0), 1.5),
}
THRESHOLD = 1.0
NAMES = sorted(CONTINUOUS)


def _inputs(f):
    """(x, x_thr, x_tanh) on the 2^-f grid.  x holds every function's breakpoints exactly, one
    unit below each, and both far ends; x_thr stays at least 4 units from the threshold."""
    u = 2.0 ** -f
    rng = np.random.default_rng(1)
    grid = lambda a: np.round(a * 2.0 ** f) / 2.0 ** f  # noqa: E731
    x = grid(rng.uniform(-8, 8, int(np.prod(SHAPE))))
    pts = sorted({t for _fn, _ref, ts, _s in CONTINUOUS.values() for t in ts})
    special = [v for t in pts for v in (t, t - u)] + [FAR, -FAR]
    x[:len(special)] = special
    xt = grid(rng.uniform(-8, 8, int(np.prod(SHAPE))))
    near = np.abs(xt - THRESHOLD) < 4 * u
    xt[near] = THRESHOLD + 8 * u
    xt[:4] = [THRESHOLD + 4 * u, THRESHOLD - 4 * u, FAR, -FAR]
    xh = grid(rng.uniform(-6, 6, int(np.prod(SHAPE))))
    return x.reshape(SHAPE), xt.reshape(SHAPE), xh.reshape(SHAPE)


def _program(ring):
    dt = DTYPES[ring]

    @pm.computation
    def prog(x: pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64)),
             xt: pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64)),
             xh: pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64))):
        with ALICE:
            xf, xtf, xhf = (pm.cast(v, dtype=dt) for v in (x, xt, xh))
        with REP:
            ys = [CONTINUOUS[n][0](xf) for n in NAMES]
            ys.append(pm.thresholded_relu(xtf, THRESHOLD))
            ys.append(pm.relu(xf))
            ys.append(pm.tanh(xhf))
        with CAROLE:
            return tuple(pm.cast(y, dtype=pm.float64) for y in ys)

    return prog


_RUNS = {}


def _evaluate_twice(device, ring):
    key = (device, ring)
    if key not in _RUNS:
        x, xt, xh = _inputs(FRAC[ring])
        kw = {"use_graphs": True} if device != "cpu" else {}
        rt = LocalMooseRuntime(ROLES, device=device, fixedpoint_ring=ring, **kw)
        comp, args = _program(ring), {"x": x, "xt": xt, "xh": xh}
        runs = []
        for _ in range(2):
            r = rt.evaluate_computation(comp, args)
            runs.append([r[f"output_{i}"] for i in range(len(NAMES) + 3)])
        _RUNS[key] = runs
    return _RUNS[key]


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("ring", (64, 128))
def test_activations_match_numpy(device, ring):
    f = FRAC[ring]
    u = 2.0 ** -f
    x, xt, _xh = _inputs(f)
    for outs in _evaluate_twice(device, ring):
        for name, got in zip(NAMES, outs):
            _fn, ref, _ts, slope = CONTINUOUS[name]
            # slope and intercept rounding, one unit of input encoding times the Lipschitz
            # constant, and TruncPr's unit
            tol = (np.abs(x).max() + slope + 3) * u
            err = np.abs(got - ref(x)).max()
            print(f"{name} ring{ring} on {device}: err {err:.3e} tol {tol:.3e}")
            assert got.shape == SHAPE and err <= tol, name
        got = outs[len(NAMES)]
        want = np.where(xt > THRESHOLD, xt, 0.0)
        tol = (np.abs(xt).max() + 1 + 3) * u
        err = np.abs(got - want).max()
        print(f"thresholded_relu ring{ring} on {device}: err {err:.3e} tol {tol:.3e}")
        assert err <= tol


@pytest.mark.parametrize("device", DEVICES)
def test_pwl_with_relu_pieces_agrees_with_relu(device):
    for ring in (64, 128):
        for outs in _evaluate_twice(device, ring):
            as_pwl, relu = outs[NAMES.index("relu_as_pwl")], outs[len(NAMES) + 1]
            assert np.abs(as_pwl - relu).max() <= 2.0 ** -FRAC[ring]


@pytest.mark.parametrize("device", DEVICES)
def test_tanh_matches_numpy(device):
    """2 * sigmoid(2x) - 1 at fixed(24, 40): twice the 1e-6 that the sigmoid keeps on |2x| <= 12
    (tests/test_reveal_precision.py), plus the units of the doubling and the constant."""
    _x, _xt, xh = _inputs(40)
    for outs in _evaluate_twice(device, 128):
        err = np.abs(outs[len(NAMES) + 2] - np.tanh(xh)).max()
        print(f"tanh on {device}: err {err:.3e}")
        assert err <= 2e-6 + 4 * 2.0 ** -40


def _tables(fn, ring):
    """The integer tables of the one PiecewiseLinear operator that ``fn`` traces to."""
    @pm.computation
    def one(x: pm.Argument(placement=ALICE, vtype=pm.TensorType(DTYPES[ring]))):
        with REP:
            y = fn(x)
        with CAROLE:
            return pm.identity(y)

    ops = [o for o in to_native(one).operations if o.kind == "PiecewiseLinear"]
    assert len(ops) == 1
    a = ops[0].attrs
    return list(a["breakpoints"]), list(a["slopes"]), list(a["intercepts"])


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("ring", (64, 128))
def test_revealed_ring_value_is_the_truncated_integer_function(device, ring):
    """Z = a_i * x + b_i * 2^f in Python integers from the operator's own tables; the opened
    value is floor(Z / 2^f) or one unit from it (TruncPr)."""
    f = FRAC[ring]
    x, xt, _xh = _inputs(f)
    cases = [(n, CONTINUOUS[n][0], x) for n in NAMES if n != "hard_swish"]
    cases.append(("thresholded_relu", lambda t: pm.thresholded_relu(t, THRESHOLD), xt))
    index = {n: i for i, n in enumerate(NAMES)}
    index["thresholded_relu"] = len(NAMES)
    for outs in _evaluate_twice(device, ring):
        for name, fn, xin in cases:
            T, A, B = _tables(fn, ring)
            xi = [int(Fraction(float(v)) * (1 << f)) for v in xin.reshape(-1)]
            gi = [int(Fraction(float(v)) * (1 << f)) for v in outs[index[name]].reshape(-1)]
            for xe, ge in zip(xi, gi):
                seg = sum(1 for t in T if xe >= t)
                z = A[seg] * xe + (B[seg] << f)
                assert abs(ge - (z >> f)) <= 1, (name, xe, ge, z >> f)


def _one_activation(ring=128):
    dt = DTYPES[ring]

    @pm.computation
    def prog(x: pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64))):
        with ALICE:
            xf = pm.cast(x, dtype=dt)
        with REP:
            y = pm.relu6(xf)
        with CAROLE:
            return pm.cast(y, dtype=pm.float64)

    return prog


def test_stacked_and_per_party_threads_reveal_equal_bits():
    comp, args = _one_activation(), {"x": _inputs(40)[0]}
    stacked = LocalMooseRuntime(ROLES, device="cpu", seed=7).evaluate_computation(comp, args)
    threads = LocalMooseRuntime(ROLES, device_map={r: "cpu" for r in ROLES},
                                seed=7).evaluate_computation(comp, args)
    assert sorted(stacked) == sorted(threads)
    for k in stacked:
        assert np.array_equal(stacked[k], threads[k])


def test_lowered_graph_takes_no_new_operator_and_agrees():
    comp, x = _one_activation(), _inputs(40)[0]
    stacked = LocalMooseRuntime(ROLES, device="cpu", seed=7).evaluate_computation(comp, {"x": x})
    low = passes.compile(to_native(comp), arg_specs={"x": x.shape})
    assert passes.is_lowered(low)
    passes.well_formed(low)
    kinds = [o.kind for o in low.operations]
    assert "PiecewiseLinear" not in kinds and kinds.count("WeightedSum") >= 9
    out = LocalMooseRuntime(ROLES, device="cpu", seed=7).evaluate_compiled(
        Computation.from_textual(low.to_textual()), {"x": x})
    for k in stacked:  # other PRF keys, so other TruncPr draws: one unit apart at most
        assert np.abs(out[k] - stacked[k]).max() <= 2.0 ** -40


def test_serialised_forms_round_trip():
    native = to_native(_one_activation())
    ops = [o for o in native.operations if o.kind == "PiecewiseLinear"]
    assert len(ops) == 1 and list(ops[0].attrs["breakpoints"]) == [0, 6 << 40]
    assert list(ops[0].attrs["slopes"]) == [0, 1 << 40, 0]
    assert list(ops[0].attrs["intercepts"]) == [0, 0, 6 << 40]
    txt = native.to_textual()
    assert "PiecewiseLinear{" in txt and f"breakpoints = [0, {6 << 40}]" in txt
    assert Computation.from_textual(txt).to_textual() == txt
    assert Computation.from_msgpack(native.to_msgpack()).to_textual() == txt
    traced = tracer.trace(_one_activation())
    pw = [o for o in traced.operations.values()
          if type(o).__name__ == "PiecewiseLinearOperation"]
    assert pw and list(pw[0].slopes) == [0, 1 << 40, 0]


def test_trace_time_errors_name_the_function():
    fx = pm.Argument(placement=ALICE, vtype=pm.TensorType(DTYPES[128]))
    fl = pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64))

    def trace(fn, arg=fx):
        @pm.computation
        def prog(x: arg):
            with REP:
                y = fn(x)
            with CAROLE:
                return pm.identity(y)

        return tracer.trace(prog)

    k = pm.edsl.base.PWL_MAX + 1
    with pytest.raises(ValueError, match="`piecewise_linear`.*breakpoints, found 9"):
        trace(lambda t: pm.piecewise_linear(t, list(range(k)), [0] * (k + 1), [0] * (k + 1)))
    with pytest.raises(ValueError, match="`piecewise_linear`.*strictly increasing"):
        trace(lambda t: pm.piecewise_linear(t, [1, 0], [0, 1, 0], [0, 0, 0]))
    with pytest.raises(ValueError, match="`piecewise_linear`.*2 breakpoints take 3 slopes"):
        trace(lambda t: pm.piecewise_linear(t, [0, 1], [0, 1], [0, 0, 0]))
    with pytest.raises(ValueError, match="`piecewise_linear`.*signed 64-bit"):
        trace(lambda t: pm.piecewise_linear(t, [0], [0, 2.0 ** 30], [0, 0]))
    with pytest.raises(ValueError, match="`clip`.*signed 64-bit"):
        trace(lambda t: pm.clip(t, 0, 2.0 ** 40))
    with pytest.raises(ValueError, match="`clip`.*not below"):
        trace(lambda t: pm.clip(t, 3, 3))
    with pytest.raises(ValueError, match="`clip` needs a lower or an upper bound"):
        trace(lambda t: pm.clip(t))
    with pytest.raises(ValueError, match="`hard_sigmoid`: alpha must be positive"):
        trace(lambda t: pm.hard_sigmoid(t, 0.0))
    for name, fn in (("piecewise_linear", lambda t: pm.piecewise_linear(t, [0], [0, 1], [0, 0])),
                     ("relu6", pm.relu6), ("clip", lambda t: pm.clip(t, 0, 1)),
                     ("leaky_relu", pm.leaky_relu), ("hard_sigmoid", pm.hard_sigmoid),
                     ("hard_tanh", pm.hard_tanh), ("thresholded_relu", pm.thresholded_relu),
                     ("hard_swish", pm.hard_swish), ("tanh", pm.tanh)):
        with pytest.raises(TypeError, match=f"`{name}` expects a fixed-point tensor"):
            trace(fn, fl)


def test_slopes_that_leave_no_headroom_are_rejected_when_run():
    """fixed(14, 23) in Z_2^64 keeps two spare bits for a slope of 1; a slope of 4 does not."""
    dt = DTYPES[64]

    @pm.computation
    def prog(x: pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64))):
        with ALICE:
            xf = pm.cast(x, dtype=dt)
        with REP:
            y = pm.piecewise_linear(xf, [0], [0, 4], [0, 0])
        with CAROLE:
            return pm.cast(y, dtype=pm.float64)

    rt = LocalMooseRuntime(ROLES, device="cpu", fixedpoint_ring=64)
    with pytest.raises(Exception, match="piecewise_linear.*Z_2\\^64"):
        rt.evaluate_computation(prog, {"x": np.zeros((2, 2))})


def test_host_fixed_point_takes_the_plain_leaf():
    dt = DTYPES[128]

    @pm.computation
    def prog(x: pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64))):
        with ALICE:
            y = pm.hard_sigmoid(pm.cast(x, dtype=dt))
            return pm.cast(y, dtype=pm.float64)

    x = _inputs(40)[0]
    got = LocalMooseRuntime(ROLES, device="cpu").evaluate_computation(prog, {"x": x})["output_0"]
    assert np.abs(got - np.clip(0.2 * x + 0.5, 0, 1)).max() <= (FAR + 0.2 + 3) * 2.0 ** -40
