"""The smooth activations (pm.gelu, silu, mish, softplus, elu, selu, celu, erf) and
pm.piecewise_polynomial: the table checks of fixedpoint.pwp_tables, the revealed values against
the operator's own integer tables in exact rationals and against float64, host placement,
per-party threads, the lowered graph, graph replays, the serialised forms and ONNX import.

Every tolerance is derived here.  B, in units of 2^-f: TruncPr leaves floor(z / 2^f) or one
more, so P_2 = x * x is within E_2 = 2 units of x^2, P_3 = P_2 * x within E_3 = ceil(L) * E_2 + 2
(L: the largest |x| of a piece with a cubic coefficient), each power's error is scaled by its
coefficient, and the last truncation adds its own 2: B = 2 + sum_{i >= 2} ceil(|c_i|max) * E_i.
Against float64 the fit error that fixedpoint.pwp_fit reports for the same tables comes on
top."""
import inspect
import math
from fractions import Fraction

import numpy as np
import pytest

import moose_amd as pm
from moose_amd.compiler import passes
from moose_amd.edsl import tracer
from moose_amd.ir.computation import Computation
from moose_amd.models import predictors
from moose_amd.models.predictors import onnx_proto as op
from moose_amd.protocols import fixedpoint as fxp
from moose_amd.runtime.local import LocalMooseRuntime
from moose_amd.runtime.local import to_native

ROLES = ["alice", "bob", "carole"]
ALICE, BOB, CAROLE = (pm.host_placement(n) for n in ROLES)
REP = pm.replicated_placement("rep", players=[ALICE, BOB, CAROLE])
# (dtype, ring, degree)
CONFIGS = {"f23": (pm.fixed(14, 23), 128, 3), "f40": (pm.fixed(24, 40), 128, 3),
           "f17q": (pm.fixed(8, 17), 64, 2)}
DEVICES = ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)]
SHAPE = (3, 7)
FAR = 20.0  # beyond every knot, inside the grid on which pwp_fit measures its error
ALPHA = 0.5
_erf = np.vectorize(math.erf, otypes=[np.float64])

# name -> (builder(x, degree), float64 reference, smooth_tables name, alpha)
FUNCTIONS = {
    "gelu": (lambda t, d: pm.gelu(t, degree=d),
             lambda v: 0.5 * v * (1 + _erf(v / math.sqrt(2))), "gelu", 1.0),
    "gelu_tanh": (lambda t, d: pm.gelu(t, approximate="tanh", degree=d),
                  lambda v: 0.5 * v * (1 + np.tanh(math.sqrt(2 / math.pi)
                                                   * (v + 0.044715 * v ** 3))),
                  "gelu_tanh", 1.0),
    "silu": (lambda t, d: pm.silu(t, degree=d), lambda v: v / (1 + np.exp(-v)), "silu", 1.0),
    "mish": (lambda t, d: pm.mish(t, degree=d),
             lambda v: v * np.tanh(np.log1p(np.exp(-np.abs(v))) + np.maximum(v, 0)), "mish", 1.0),
    "softplus": (lambda t, d: pm.softplus(t, degree=d),
                 lambda v: np.log1p(np.exp(-np.abs(v))) + np.maximum(v, 0), "softplus", 1.0),
    "elu": (lambda t, d: pm.elu(t, ALPHA, degree=d),
            lambda v: np.where(v > 0, v, ALPHA * (np.exp(np.minimum(v, 0)) - 1)), "elu", ALPHA),
    "selu": (lambda t, d: pm.selu(t, degree=d),
             lambda v: 1.0507009873554805 * np.where(
                 v > 0, v, 1.6732632423543772 * (np.exp(np.minimum(v, 0)) - 1)), "selu", 1.0),
    "celu": (lambda t, d: pm.celu(t, ALPHA, degree=d),
             lambda v: np.maximum(v, 0) + np.minimum(
                 0, ALPHA * (np.exp(np.minimum(v, 0) / ALPHA) - 1)), "celu", ALPHA),
    "erf": (lambda t, d: pm.erf(t, degree=d), _erf, "erf", 1.0),
}
NAMES = sorted(FUNCTIONS)


def test_swish_is_silu():
    assert pm.swish is pm.silu


# ---------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------
def _int_tables(name, cfg):
    """(T, rows, fit_err): the integer tables that ``name`` traces to at the configuration's
    precision and the error pwp_fit reports for exactly those tables."""
    dt, _ring, deg = CONFIGS[cfg]
    f = dt.fractional_precision
    _fn, _ref, fit_name, alpha = FUNCTIONS[name]
    T, C, err = fxp.smooth_tables(fit_name, alpha, deg, 8, f)
    enc = lambda v: int(Fraction(v) * (1 << f))  # noqa: E731  (exact: rounded to 2^-f)
    for v in list(T) + [c for row in C for c in row]:
        assert Fraction(v) * (1 << f) == enc(v)
    return [enc(t) for t in T], [[enc(c) for c in row] for row in C], err


def _bound(T, rows, f):
    """B of the module docstring, from the integer tables."""
    d = len(rows[0]) - 1
    E = {2: 2}
    if d == 3:
        cubic = [j for j, row in enumerate(rows) if row[3]]
        assert cubic and 0 not in cubic and len(T) not in cubic  # the outer pieces are linear
        L = max(max(abs(T[j - 1]), abs(T[j])) for j in cubic)
        E[3] = -(-L >> f) * E[2] + 2
    return 2 + sum(-(-max(abs(row[i]) for row in rows) >> f) * E[i] for i in range(2, d + 1))


def _spline_units(T, rows, f, xi):
    """The integer-table spline at the ring integer xi, in units of 2^-f, as a Fraction."""
    seg = sum(1 for t in T if xi >= t)
    return sum(Fraction(c * xi ** i, 1 << (f * i)) for i, c in enumerate(rows[seg]))


def test_pwp_tables_rejections_name_the_bits():
    ok_T, ok_C = [-(1 << 23), 1 << 23], [[0, 0, 0], [0, 1 << 23, 1 << 20], [0, 1 << 23, 0]]
    T, D, CK, C0K = fxp.pwp_tables(ok_T, ok_C, 23, 14, 128)
    assert T == ok_T and len(D) == 3 and CK == [1 << 23, 0] and C0K == 0
    assert D[1] == [-(1 << 23), 0] and D[2] == [-(1 << 20), 1 << 20]
    with pytest.raises(ValueError, match="strictly increasing"):
        fxp.pwp_tables([1, 1], ok_C, 23, 14, 128)
    with pytest.raises(ValueError, match="strictly increasing"):
        fxp.pwp_tables([2, 1], ok_C, 23, 14, 128)
    nine = list(range(9))
    with pytest.raises(ValueError, match="between 1 and 8 breakpoints.*found 9"):
        fxp.pwp_tables(nine, [[0, 1]] * 10, 23, 14, 128)
    with pytest.raises(ValueError, match="one more coefficient row"):
        fxp.pwp_tables(ok_T, ok_C[:2], 23, 14, 128)
    with pytest.raises(ValueError, match="degree d between 1 and 3"):
        fxp.pwp_tables(ok_T, [[0] * 5] * 3, 23, 14, 128)
    # a cubic on fixed(24, 40) over Z_2^64: x alone takes 64 bits, its powers more
    T, C, _err = _int_tables("gelu", "f40")
    with pytest.raises(ValueError, match=r"needs \d+ bits before.*Z_2\^64 leaves 62"):
        fxp.pwp_tables(T, C, 40, 24, 64)
    # the power alone: |x| <= 2^10 cubed at f = 23 needs 30 + 23 + 23 + 1 bits
    big = [[0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0]]
    with pytest.raises(ValueError, match=r"power x\^3.*needs 7[0-9] bits before its truncation, "
                                         r"but Z_2\^64 leaves 62"):
        fxp.pwp_tables([-(1 << 33), 1 << 33], big, 23, 14, 64)
    # every shipped function fits its configuration
    for cfg, (dt, ring, _deg) in CONFIGS.items():
        for name in NAMES:
            T, C, _err = _int_tables(name, cfg)
            fxp.pwp_tables(T, C, dt.fractional_precision, dt.integral_precision, ring)


def test_pwp_fit_is_deterministic_and_reports_its_own_error():
    fn, tails, kinks = fxp.smooth_function("elu", ALPHA)
    a = fxp.pwp_fit(fn, 3, 8, tails, kinks)
    b = fxp.pwp_fit(fn, 3, 8, tails, kinks)
    assert a == b
    T, C, err = a
    assert 0.0 in T and len(T) == 8 and len(C) == 9 and all(len(r) == 4 for r in C)
    assert C[0] == [-ALPHA, 0.0, 0.0, 0.0] and C[-1] == [0.0, 1.0, 0.0, 0.0]
    grid = np.linspace(-24, 24, 9601)
    seg = np.searchsorted(np.asarray(T), grid, side="right")
    got = sum(np.asarray(C)[seg, i] * grid ** i for i in range(4))
    assert np.abs(got - FUNCTIONS["elu"][1](grid)).max() <= err
    with pytest.raises(ValueError, match="degree of 1, 2 or 3"):
        fxp.pwp_fit(fn, 4, 8, tails, kinks)
    with pytest.raises(ValueError, match="breakpoints, found 9"):
        fxp.pwp_fit(fn, 3, 9, tails, kinks)


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
def _inputs(name, cfg):
    """[3, 7] on the 2^-f grid: every knot, one unit below every knot, one unit above the
    first and the last, far in both tails, and 0."""
    f = CONFIGS[cfg][0].fractional_precision
    T, _rows, _err = _int_tables(name, cfg)
    far = int(FAR * (1 << f))
    xi = list(T) + [t - 1 for t in T] + [T[0] + 1, T[-1] + 1, far, -far, 0]
    assert len(T) == 8 and len(xi) == SHAPE[0] * SHAPE[1]
    return np.array([v / (1 << f) for v in xi]).reshape(SHAPE), xi


def _program(cfg):
    dt, _ring, deg = CONFIGS[cfg]
    arg = pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64))

    def body(*xs):
        with ALICE:
            xf = [pm.cast(x, dtype=dt) for x in xs]
            hs = [FUNCTIONS[n][0](x, deg) for n, x in zip(NAMES, xf)]
            hs = [pm.cast(h, dtype=pm.float64) for h in hs]
        with REP:
            ys = [FUNCTIONS[n][0](x, deg) for n, x in zip(NAMES, xf)]
        with CAROLE:
            return tuple(pm.cast(y, dtype=pm.float64) for y in ys) + tuple(
                pm.identity(h) for h in hs)

    # one float64 argument per function, named after it
    params = [inspect.Parameter(n, inspect.Parameter.POSITIONAL_OR_KEYWORD, annotation=arg)
              for n in NAMES]
    body.__signature__ = inspect.Signature(params)
    body.__name__ = f"smooth_{cfg}"
    return pm.computation(body)


_RUNS = {}


def _evaluate(device, cfg):
    """Three seeded evaluations of the configuration's program (on a GPU with hipGraphs: the
    second and the third are replays); each -> (replicated outputs, host outputs)."""
    key = (device, cfg)
    if key not in _RUNS:
        _dt, ring, _deg = CONFIGS[cfg]
        kw = {"use_graphs": True} if device != "cpu" else {}
        rt = LocalMooseRuntime(ROLES, device=device, fixedpoint_ring=ring, seed=5, **kw)
        comp, args = _program(cfg), {n: _inputs(n, cfg)[0] for n in NAMES}
        runs = []
        for _ in range(3):
            r = rt.evaluate_computation(comp, args)
            outs = [r[f"output_{i}"] for i in range(2 * len(NAMES))]
            runs.append((outs[:len(NAMES)], outs[len(NAMES):]))
        _RUNS[key] = runs
    return _RUNS[key]


def _units(a, f):
    return [int(Fraction(float(v)) * (1 << f)) for v in np.asarray(a).reshape(-1)]


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_revealed_values_match_the_integer_spline_and_float64(device, cfg):
    f = CONFIGS[cfg][0].fractional_precision
    rep_outs, _host = _evaluate(device, cfg)[0]
    for name, got in zip(NAMES, rep_outs):
        T, rows, fit_err = _int_tables(name, cfg)
        B = _bound(T, rows, f)
        x, xi = _inputs(name, cfg)
        assert got.shape == SHAPE
        worst = max(abs(g - _spline_units(T, rows, f, v)) for g, v in zip(_units(got, f), xi))
        err = np.abs(got - FUNCTIONS[name][1](x)).max()
        print(f"{name} {cfg} on {device}: {float(worst):.2f} units of B = {B}; float64 err "
              f"{err:.3e}, fit {fit_err:.3e}")
        assert worst <= B, name
        assert err <= B * 2.0 ** -f + fit_err, name


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_host_placement_agrees_with_replicated(device, cfg):
    f = CONFIGS[cfg][0].fractional_precision
    rep_outs, host_outs = _evaluate(device, cfg)[0]
    for name, r, h in zip(NAMES, rep_outs, host_outs):
        T, rows, _err = _int_tables(name, cfg)
        B = _bound(T, rows, f)
        _x, xi = _inputs(name, cfg)
        # the host's own arithmetic-shift truncations stay inside B of the exact spline
        assert max(abs(g - _spline_units(T, rows, f, v))
                   for g, v in zip(_units(h, f), xi)) <= B, name
        assert max(abs(a - b) for a, b in zip(_units(r, f), _units(h, f))) <= B, name


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_second_and_third_evaluation_equal_the_first_bitwise(device, cfg):
    first, second, third = _evaluate(device, cfg)
    for later in (second, third):
        for a, b in zip(first[0] + first[1], later[0] + later[1]):
            assert np.array_equal(a, b)


def _one_activation(cfg="f40", where=REP):
    dt, _ring, deg = CONFIGS[cfg]

    @pm.computation
    def prog(x: pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64))):
        with ALICE:
            xf = pm.cast(x, dtype=dt)
        with where:
            y = pm.gelu(xf, degree=deg)
        with CAROLE:
            return pm.cast(y, dtype=pm.float64)

    return prog


def test_stacked_and_per_party_threads_reveal_equal_bits():
    for cfg in ("f40", "f17q"):
        ring = CONFIGS[cfg][1]
        comp, args = _one_activation(cfg), {"x": _inputs("gelu", cfg)[0]}
        stacked = LocalMooseRuntime(ROLES, device="cpu", seed=7,
                                    fixedpoint_ring=ring).evaluate_computation(comp, args)
        threads = LocalMooseRuntime(ROLES, device_map={r: "cpu" for r in ROLES}, seed=7,
                                    fixedpoint_ring=ring).evaluate_computation(comp, args)
        assert sorted(stacked) == sorted(threads)
        for k in stacked:
            assert np.array_equal(stacked[k], threads[k])


def test_lowered_graph_takes_no_new_operator_and_agrees():
    f = 40
    comp, (x, _xi) = _one_activation(), _inputs("gelu", "f40")
    T, rows, _err = _int_tables("gelu", "f40")
    B = _bound(T, rows, f)
    eager = LocalMooseRuntime(ROLES, device="cpu", seed=7).evaluate_computation(comp, {"x": x})
    low = passes.compile(to_native(comp), arg_specs={"x": x.shape})
    assert passes.is_lowered(low)
    passes.well_formed(low)
    kinds = [o.kind for o in low.operations]
    assert "PiecewisePolynomial" not in kinds and kinds.count("WeightedSum") >= 3 * 7
    out = LocalMooseRuntime(ROLES, device="cpu", seed=7).evaluate_compiled(
        Computation.from_textual(low.to_textual()), {"x": x})
    for k in eager:  # other PRF keys, so other TruncPr draws
        assert max(abs(a - b) for a, b in zip(_units(out[k], f), _units(eager[k], f))) <= B


def test_serialised_forms_round_trip():
    native = to_native(_one_activation())
    ops = [o for o in native.operations if o.kind == "PiecewisePolynomial"]
    T, rows, _err = _int_tables("gelu", "f40")
    assert len(ops) == 1 and list(ops[0].attrs["breakpoints"]) == T
    assert list(ops[0].attrs["coefficients"]) == [c for row in rows for c in row]
    assert ops[0].attrs["degree"] == 3
    txt = native.to_textual()
    assert "PiecewisePolynomial{" in txt and f"breakpoints = [{T[0]}, {T[1]}," in txt
    assert "degree = 3" in txt
    assert Computation.from_textual(txt).to_textual() == txt
    assert Computation.from_msgpack(native.to_msgpack()).to_textual() == txt
    traced = tracer.trace(_one_activation())
    pw = [o for o in traced.operations.values()
          if type(o).__name__ == "PiecewisePolynomialOperation"]
    assert pw and list(pw[0].breakpoints) == T and pw[0].degree == 3


def test_piecewise_polynomial_takes_real_tables():
    """x^2 on [-2, 2), 4 outside, at fixed(14, 23): exact up to the two truncations."""
    dt = CONFIGS["f23"][0]

    @pm.computation
    def prog(x: pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64))):
        with ALICE:
            xf = pm.cast(x, dtype=dt)
        with REP:
            y = pm.piecewise_polynomial(xf, [-2, 2], [[4, 0, 0], [0, 0, 1], [4, 0, 0]])
        with CAROLE:
            return pm.cast(y, dtype=pm.float64)

    x = np.array([-3.0, -2.0, -1.5, 0.0, 0.25, 1.999, 2.0, 7.0])
    got = LocalMooseRuntime(ROLES, device="cpu").evaluate_computation(prog, {"x": x})["output_0"]
    want = np.where(np.abs(x) < 2, x * x, 4.0)
    want[1] = 4.0  # -2 is in the middle piece: (-2)^2
    # E_2 = 2 units scaled by the coefficient 1, the last truncation's 2, and the input's
    # rounding to the grid scaled by the slope |2x| <= 4
    assert np.abs(got - want).max() <= (2 + 2 + 4) * 2.0 ** -23


def test_trace_time_errors_name_the_function():
    fx = pm.Argument(placement=ALICE, vtype=pm.TensorType(CONFIGS["f40"][0]))
    fl = pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64))

    def trace(fn, arg=fx):
        @pm.computation
        def prog(x: arg):
            with REP:
                y = fn(x)
            with CAROLE:
                return pm.identity(y)

        return tracer.trace(prog)

    with pytest.raises(ValueError, match="`piecewise_polynomial`.*breakpoints, found 9"):
        trace(lambda t: pm.piecewise_polynomial(t, list(range(9)), [[0, 1]] * 10))
    with pytest.raises(ValueError, match="`piecewise_polynomial`.*strictly increasing"):
        trace(lambda t: pm.piecewise_polynomial(t, [1, 0], [[0, 1]] * 3))
    with pytest.raises(ValueError, match="`piecewise_polynomial`.*2 breakpoints take 3"):
        trace(lambda t: pm.piecewise_polynomial(t, [0, 1], [[0, 1]] * 2))
    with pytest.raises(ValueError, match="`piecewise_polynomial`.*degree 1 to 3"):
        trace(lambda t: pm.piecewise_polynomial(t, [0], [[0] * 5] * 2))
    with pytest.raises(ValueError, match="`gelu`: approximate"):
        trace(lambda t: pm.gelu(t, approximate="fast"))
    with pytest.raises(ValueError, match="`silu`: a degree of 1, 2 or 3"):
        trace(lambda t: pm.silu(t, degree=4))
    with pytest.raises(ValueError, match="`mish`: between 2 and 8 breakpoints"):
        trace(lambda t: pm.mish(t, pieces=9))
    with pytest.raises(ValueError, match="`celu`: alpha must not be zero"):
        trace(lambda t: pm.celu(t, 0.0))
    for name in ("gelu", "silu", "swish", "mish", "softplus", "elu", "selu", "celu", "erf"):
        with pytest.raises(TypeError, match="expects a fixed-point tensor"):
            trace(getattr(pm, name), fl)


def test_tables_that_leave_no_headroom_are_rejected_when_run():
    @pm.computation
    def prog(x: pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64))):
        with ALICE:
            xf = pm.cast(x, dtype=pm.fixed(24, 40))
        with REP:
            y = pm.gelu(xf)
        with CAROLE:
            return pm.cast(y, dtype=pm.float64)

    rt = LocalMooseRuntime(ROLES, device="cpu", fixedpoint_ring=64)
    with pytest.raises(Exception, match=r"piecewise_polynomial.*Z_2\^64 leaves 62"):
        rt.evaluate_computation(prog, {"x": np.zeros((2, 2))})


# ---------------------------------------------------------------------------
# ONNX
# ---------------------------------------------------------------------------
RNG = np.random.default_rng(41)
f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)  # noqa: E731
W1, B1 = f32(RNG.uniform(-1.0, 1.0, (3, 2, 3, 3))), f32(RNG.uniform(-0.5, 0.5, 3))
WD, BD = f32(RNG.uniform(-0.5, 0.5, (5, 3 * 4 * 4))), f32(RNG.uniform(-0.5, 0.5, 5))
X = np.random.default_rng(42).uniform(-1, 1, (2, 2, 4, 4))
INITS = {"w1": W1, "b1": B1, "wd": WD, "bd": BD}
SELU_A, SELU_G = 1.6732632423543772, 1.0507009873554805
# ONNX activation -> (attributes, float64 reference key, fitted name, alpha)
ONNX_ACTS = {"Mish": ({}, "mish", "mish", 1.0), "Softplus": ({}, "softplus", "softplus", 1.0),
             "Elu": ({"alpha": ALPHA}, "elu", "elu", ALPHA), "Selu": ({}, "selu", "selu", 1.0),
             "Erf": ({}, "erf", "erf", 1.0)}


def _tensor(name, a):
    a = np.asarray(a).astype(np.float32)
    return op.make("TensorProto", name=name, dims=list(a.shape), data_type=1,
                   raw_data=a.tobytes())


def _node(kind, ins, out, **attrs):
    return op.make("NodeProto", input=list(ins), output=[out], name=f"{kind}_{out}",
                   op_type=kind, attribute=[op.attr(k, v) for k, v in attrs.items()])


def _model(nodes, opset=20):
    dims = [op.make("Dimension", dim_param="N")] + [op.make("Dimension", dim_value=d)
                                                    for d in (2, 4, 4)]
    inp = op.make("ValueInfoProto", name="x", type=op.make(
        "TypeProto", tensor_type=op.make("TypeProtoTensor", elem_type=1,
                                         shape=op.make("TensorShapeProto", dim=dims))))
    out = op.make("ValueInfoProto", name="y", type=op.make(
        "TypeProto", tensor_type=op.make("TypeProtoTensor", elem_type=1)))
    graph = op.make("GraphProto", node=nodes, name="net", input=[inp], output=[out],
                    initializer=[_tensor(k, v) for k, v in INITS.items()])
    return op.serialize(op.make("ModelProto", ir_version=9, producer_name="pytorch",
                                producer_version="2.3", graph=graph,
                                opset_import=[op.make("OperatorSetIdProto", domain="",
                                                      version=opset)]))


def _net(act=None, opset=20, gelu_attrs=None, **act_attrs):
    """Conv -> Gelu -> Flatten -> Gemm, then ``act`` on the dense output."""
    nodes = [
        _node("Conv", ["x", "w1", "b1"], "c1", kernel_shape=[3, 3], pads=[1, 1, 1, 1]),
        _node("Gelu", ["c1"], "a1", **(gelu_attrs or {})),
        _node("Flatten", ["a1"], "f", axis=1),
        _node("Gemm", ["f", "wd", "bd"], "g" if act else "y", transB=1),
    ]
    if act:
        nodes.append(_node(act, ["g"], "y", **act_attrs))
    return _model(nodes, opset)


def _lipschitz(ref):
    grid = np.linspace(-24, 24, 48001)
    return float(np.abs(np.diff(ref(grid)) / np.diff(grid)).max())


def _activation_error(fit_name, alpha, ref, err_in, f=40):
    """What a smooth activation makes of an input error: its slope times it, plus B units
    and the fit error of its own tables (cubic, 8 breakpoints, fixed(24, 40))."""
    T, C, fit_err = fxp.smooth_tables(fit_name, alpha, 3, 8, f)
    enc = lambda v: int(Fraction(v) * (1 << f))  # noqa: E731
    B = _bound([enc(t) for t in T], [[enc(c) for c in row] for row in C], f)
    return _lipschitz(ref) * err_in + B * 2.0 ** -f + fit_err


def _forward(act, approximate="none"):
    """The float64 forward pass and the tolerance summed over the layers: every product
    layer scales the error by its largest absolute row sum and adds half a unit per weight
    (its rounding) times the largest input, plus TruncPr's 2 units."""
    u = 2.0 ** -40
    xp = np.pad(X, ((0, 0), (0, 0), (1, 1), (1, 1)))
    c1 = np.zeros((X.shape[0], 3, 4, 4))
    for i in range(4):
        for j in range(4):
            c1[:, :, i, j] = np.einsum("nchw,ochw->no", xp[:, :, i:i + 3, j:j + 3], W1) + B1
    err = u / 2  # the input's encoding
    err = np.abs(W1).reshape(3, -1).sum(1).max() * err + W1[0].size * np.abs(X).max() * u / 2 \
        + 3 * u
    gelu = FUNCTIONS["gelu" if approximate == "none" else "gelu_tanh"]
    a1 = gelu[1](c1)
    err = _activation_error(gelu[2], 1.0, gelu[1], err)
    g = a1.reshape(X.shape[0], -1) @ WD.T + BD
    err = np.abs(WD).sum(1).max() * err + WD.shape[1] * np.abs(a1).max() * u / 2 + 3 * u
    if act is None:
        return g, err
    _attrs, ref_key, fit_name, alpha = ONNX_ACTS[act]
    ref = FUNCTIONS[ref_key][1]
    return ref(g), _activation_error(fit_name, alpha, ref, err)


def _check_onnx(device, cases):
    kw = {"use_graphs": True} if device != "cpu" else {}
    for act, approximate in cases:
        attrs = ONNX_ACTS[act][0] if act else {}
        net = predictors.from_onnx(_net(act, gelu_attrs={"approximate": approximate}, **attrs))
        want, tol = _forward(act, approximate)
        rt = LocalMooseRuntime(ROLES, device=device, **kw)
        comp = net.predictor_factory()
        for _ in range(2):  # with hipGraphs the second evaluation is a replay
            got = rt.evaluate_computation(comp, {"x": X})["output_0"]
            err = np.abs(got - want).max()
            print(f"Gelu({approximate}) -> {act} on {device}: err {err:.3e} tol {tol:.3e}")
            assert got.shape == want.shape and err <= tol, (act, approximate)


ONNX_CASES = [(None, "tanh")] + [(a, "none") for a in sorted(ONNX_ACTS)]


def test_onnx_models_match_numpy_cpu():
    _check_onnx("cpu", ONNX_CASES)


@pytest.mark.gpu
def test_onnx_models_match_numpy_gpu():
    _check_onnx("cuda:0", ONNX_CASES)


def test_onnx_layers_and_rejections_name_the_node():
    net = predictors.from_onnx(_net("Elu", alpha=ALPHA))
    assert [l["op"] for l in net.layers] == ["conv", "gelu", "flatten", "dense", "elu"]
    assert net.layers[1]["approximate"] == "none" and net.layers[4]["alpha"] == ALPHA
    assert predictors.from_onnx(_net("Celu", alpha=2.0)).layers[4] == {"op": "celu", "alpha": 2.0}
    assert predictors.from_onnx(_net("Swish", opset=24)).layers[4] == {"op": "silu"}
    with pytest.raises(ValueError, match="Gelu_a1.*approximate='fast'"):
        predictors.from_onnx(_net(gelu_attrs={"approximate": "fast"}))
    with pytest.raises(ValueError, match="Mish_y.*unsupported attribute.*alpha"):
        predictors.from_onnx(_net("Mish", alpha=1.0))
    with pytest.raises(ValueError, match="Selu_y.*only the default"):
        predictors.from_onnx(_net("Selu", alpha=1.0))
    with pytest.raises(ValueError, match="Swish_y.*alpha=2.0"):
        predictors.from_onnx(_net("Swish", opset=24, alpha=2.0))
    # a model of an opset that has no Gelu yet keeps its rejection
    with pytest.raises(ValueError, match="Gelu_a1.*not an operator of opset 15.*opset 20"):
        predictors.from_onnx(_net(opset=15))
