"""The Python eDSL: placements, arguments, expressions and op builders.

API-compatible with ``pymoose.edsl.base`` (reference ``pymoose/pymoose/edsl/base.py``,
49 op builders at ``:611-1771``).  Where the reference defines one Expression
dataclass per op, here every expression is a single :class:`Expression` record with an
op ``kind`` and an ``attrs`` dict; the tracer (``tracer.py``) maps kinds to IR
operations through one table.
"""
from __future__ import annotations

import builtins
import functools as ft
import inspect
from dataclasses import dataclass
from dataclasses import field
from fractions import Fraction
from typing import Any
from typing import Dict
from typing import List
from typing import Optional

import numpy as np

from moose_amd.computation import dtypes
from moose_amd.computation import types as ty
from moose_amd.computation import values

EllipsisType = type(...)

CURRENT_PLACEMENT: List = []
_CURRENT_RUNTIME = None

_NUMPY_DTYPES_MAP = {
    np.dtype("uint32"): dtypes.uint32,
    np.dtype("uint64"): dtypes.uint64,
    np.dtype("int32"): dtypes.int32,
    np.dtype("int64"): dtypes.int64,
    np.dtype("float32"): dtypes.float32,
    np.dtype("float64"): dtypes.float64,
    np.dtype("bool"): dtypes.bool_,
}


def _np_to_moose_dtype(d):
    try:
        return _NUMPY_DTYPES_MAP.get(np.dtype(d))
    except TypeError:
        return None


def get_current_runtime():
    return _CURRENT_RUNTIME


def set_current_runtime(runtime):
    global _CURRENT_RUNTIME
    _CURRENT_RUNTIME = runtime


# ---------------------------------------------------------------------------
# placements
# ---------------------------------------------------------------------------
@dataclass
class PlacementExpression:
    name: str

    def __enter__(self):
        CURRENT_PLACEMENT.append(self)
        return self

    def __exit__(self, *exc):
        CURRENT_PLACEMENT.pop(-1)

    def __hash__(self):
        return hash(self.name)


@dataclass(eq=True)
class HostPlacementExpression(PlacementExpression):
    def __hash__(self):
        return hash(self.name)


@dataclass(eq=True)
class MirroredPlacementExpression(PlacementExpression):
    players: List[PlacementExpression] = field(default_factory=list)

    def __hash__(self):
        return hash(self.name)


@dataclass(eq=True)
class ReplicatedPlacementExpression(PlacementExpression):
    players: List[PlacementExpression] = field(default_factory=list)

    def __hash__(self):
        return hash(self.name)


def host_placement(name):
    return HostPlacementExpression(name=name)


def mirrored_placement(name, players):
    return MirroredPlacementExpression(name=name, players=list(players))


def replicated_placement(name, players):
    return ReplicatedPlacementExpression(name=name, players=list(players))


def get_current_placement():
    return CURRENT_PLACEMENT[-1]


def _materialize_placement_arg(plc):
    plc = plc or get_current_placement()
    if not isinstance(plc, PlacementExpression):
        raise TypeError(f"Expected value of type Placement, found {type(plc)}.")
    return plc


# ---------------------------------------------------------------------------
# arguments and expressions
# ---------------------------------------------------------------------------
@dataclass(init=False)
class Argument:
    """Type annotation for computation parameters (placement + value type)."""

    placement: PlacementExpression
    dtype: Optional[dtypes.DType] = None
    vtype: Optional[ty.ValueType] = None

    def __init__(self, placement, dtype=None, vtype=None, shape=None):
        self.placement = placement
        self.dtype = dtype
        self.vtype = _maybe_lift_dtype_to_tensor_vtype(dtype, vtype)
        # optional static shape (None for a dimension only known at run time): what the
        # shape-dependent builders (conv2d, pooling) read when it is given
        self.shape = None if shape is None else tuple(shape)


@dataclass(eq=False)
class Expression:
    """One node of the traced expression DAG.

    ``kind`` names the op (``"add"``, ``"dot"``, ``"cast"`` ...); ``attrs`` carries its
    static attributes (``axis``, ``tag`` ...).
    """

    kind: str
    placement: PlacementExpression
    inputs: List["Expression"]
    vtype: Optional[ty.ValueType]
    attrs: Dict[str, Any] = field(default_factory=dict)
    # statically known shape, where a builder could tell (None entries: run-time sizes)
    static_shape: Optional[tuple] = None

    def __hash__(self):
        return id(self)

    def __getattr__(self, item):
        # attribute sugar: expr.axis, expr.tag, expr.arg_name ...
        attrs = self.__dict__.get("attrs")
        if attrs is not None and item in attrs:
            return attrs[item]
        raise AttributeError(item)

    # slicing sugar
    def __getitem__(self, slice_spec):
        if isinstance(self.vtype, (ty.TensorType, ty.AesTensorType)):
            if isinstance(slice_spec, (slice, EllipsisType)):
                slice_spec = (slice_spec,)
            if not isinstance(slice_spec, (list, tuple)):
                raise ValueError("Tensor indexing expects slices or Ellipsis")
            rewritten = []
            for s in slice_spec:
                if isinstance(s, EllipsisType):
                    rewritten.append(slice(None, None, None))
                elif isinstance(s, slice):
                    rewritten.append(s)
                else:
                    raise ValueError(
                        "Indexing with other types different than Ellipsis and slice "
                        "is not yet supported."
                    )
            return strided_slice(self, slices=rewritten)
        if isinstance(self.vtype, ty.ShapeType):
            if isinstance(slice_spec, (tuple, list)):
                if len(slice_spec) != 2:
                    raise ValueError("Indexing ShapeType requires a simple slice.")
                begin, end = slice_spec
            elif isinstance(slice_spec, slice):
                if slice_spec.step is not None:
                    raise ValueError("Indexing ShapeType requires a simple slice.")
                begin, end = slice_spec.start, slice_spec.stop
            else:
                raise ValueError("Indexing ShapeType requires a simple slice.")
            return sliced(self, begin, end)
        raise IndexError(f"Expression of vtype {self.vtype} is not slice-able.")

    # arithmetic sugar
    def __neg__(self):
        _check_arithmetickable(self, "negate")
        if isinstance(self.vtype, ty.TensorType) and not self.vtype.dtype.is_signed:
            raise TypeError(f"Cannot negate Tensor of unsigned DType {self.vtype.dtype}.")
        return mul(constant(-1, vtype=self.vtype), self)

    def __abs__(self):
        _check_arithmetickable(self, "abs")
        if isinstance(self.vtype, ty.TensorType) and not self.vtype.dtype.is_signed:
            return self
        return abs(self)

    def __add__(self, o):
        return _dunder(self, o, add, "add")

    def __radd__(self, o):
        return _dunder(o, self, add, "add")

    def __sub__(self, o):
        return _dunder(self, o, sub, "subtract")

    def __rsub__(self, o):
        return _dunder(o, self, sub, "subtract")

    def __mul__(self, o):
        return _dunder(self, o, mul, "multiply")

    def __rmul__(self, o):
        return _dunder(o, self, mul, "multiply")

    def __truediv__(self, o):
        return _dunder(self, o, div, "divide")

    def __rtruediv__(self, o):
        return _dunder(o, self, div, "divide")

    def __matmul__(self, o):
        return _dunder(self, o, dot, "dot-product")

    def __rmatmul__(self, o):
        return _dunder(o, self, dot, "dot-product")

    def __gt__(self, o):
        return _dunder(self, o, greater, "greater-than")

    def __lt__(self, o):
        return _dunder(self, o, less, "less-than")

    __iadd__ = __add__
    __isub__ = __sub__
    __imul__ = __mul__
    __itruediv__ = __truediv__
    __imatmul__ = __matmul__


def _dunder(x, y, fn, desc):
    _check_arithmetickable(x, desc)
    _check_arithmetickable(y, desc)
    return fn(x, y)


def _check_arithmetickable(expr, fn_name):
    if not isinstance(expr, Expression) or not isinstance(
        expr.vtype, (ty.TensorType, ty.FloatType, ty.IntType)
    ):
        raise TypeError(f"Value of vtype {getattr(expr, 'vtype', expr)} is not {fn_name}-able.")


# builders whose result has the shape of their (first) operand
_SAME_SHAPE = {"identity", "cast", "exp", "sqrt", "sigmoid", "relu", "log", "log2", "abs",
               "softmax", "piecewise_linear", "piecewise_polynomial"}


def _expr(kind, inputs, vtype, placement, **attrs):
    inputs = list(inputs)
    shape = None
    if kind in _SAME_SHAPE and inputs and isinstance(inputs[0], Expression):
        shape = inputs[0].static_shape
    return Expression(
        kind=kind,
        placement=_materialize_placement_arg(placement),
        inputs=inputs,
        vtype=vtype,
        attrs=attrs,
        static_shape=shape,
    )


# ---------------------------------------------------------------------------
# type helpers
# ---------------------------------------------------------------------------
def _assimilate_arg_vtypes(lhs_vtype, rhs_vtype, fn_name):
    if isinstance(lhs_vtype, ty.TensorType) and isinstance(rhs_vtype, ty.TensorType):
        if lhs_vtype.dtype != rhs_vtype.dtype:
            raise ValueError(
                f"Function `{fn_name}` expected arguments of similar dtype: "
                f"found mismatched dtypes `{lhs_vtype.dtype}` and `{rhs_vtype.dtype}`."
            )
        return lhs_vtype
    if lhs_vtype != rhs_vtype:
        raise ValueError(
            f"Function `{fn_name}` expected arguments of similar type: "
            f"found mismatched types `{lhs_vtype}` and `{rhs_vtype}`."
        )
    return lhs_vtype


def _maybe_lift_dtype_to_tensor_vtype(dtype, vtype):
    if dtype is None:
        return vtype
    if vtype is None:
        return ty.TensorType(dtype)
    if isinstance(vtype, ty.TensorType) and vtype.dtype != dtype:
        raise ValueError(
            f"Inconsistent type information for tensor: dtype {dtype} is "
            f"inconsistent with tensor type {vtype}."
        )
    return vtype


def _check_array_args(arrays, fn):
    if not isinstance(arrays, (tuple, list)):
        raise ValueError(
            f"Inputs to `{fn}` must be array-like, found argument of type {type(arrays)}."
        )
    vt = arrays[0].vtype
    if not isinstance(vt, ty.TensorType):
        raise ValueError(f"Inputs must be have vtype TensorType, found {vt}.")
    for a in arrays:
        if not isinstance(a.vtype, ty.TensorType) or a.vtype.dtype != vt.dtype:
            raise ValueError(
                f"Values passed to {fn} must be same dtype: found {a.vtype} and {vt}."
            )
    return vt


def _shape_operand(shape, placement):
    """Lift a python list/tuple shape into a host-placed ShapeConstant."""
    if isinstance(shape, (list, tuple)):
        plc = _materialize_placement_arg(placement)
        host = plc.players[0] if isinstance(plc, ReplicatedPlacementExpression) else plc
        return constant(values.ShapeConstant(value=tuple(shape)), vtype=ty.ShapeType(),
                        placement=host)
    assert isinstance(shape, Expression)
    return shape


# ---------------------------------------------------------------------------
# op builders
# ---------------------------------------------------------------------------
def add_n(arrays, placement=None):
    """Elementwise sum of a list of tensors."""
    vt = _check_array_args(arrays, "add_n")
    return _expr("add_n", arrays, vt, placement)


def identity(x, placement=None):
    """Identity; may move ``x`` to another placement."""
    return _expr("identity", [x], x.vtype, placement)


def concatenate(arrays, axis=0, placement=None):
    """Concatenate tensors along an existing ``axis``."""
    vt = _check_array_args(arrays, "concatenate")
    return _expr("concatenate", arrays, vt, placement, axis=axis)


def maximum(arrays, placement=None):
    """Elementwise maximum of a list of tensors."""
    vt = _check_array_args(arrays, "maximum")
    return _expr("maximum", arrays, vt, placement)


def decrypt(key, ciphertext, placement=None):
    """AES-GCM decrypt ``ciphertext`` (AesTensorType) with ``key`` (AesKeyType)."""
    if not isinstance(key.vtype, ty.AesKeyType):
        raise ValueError(f"Parameter `key` expected to be of type AesKeyType, found {key.vtype}.")
    if not isinstance(ciphertext.vtype, ty.AesTensorType):
        raise ValueError(
            f"Parameter `ciphertext` expected to be of type AesTensorType, found {ciphertext.vtype}."
        )
    return _expr("decrypt", [key, ciphertext], ty.TensorType(ciphertext.vtype.dtype),
                 placement)


def constant(value, dtype=None, vtype=None, placement=None):
    """Embed a constant (python scalar, string, ndarray or Shape/other Constant)."""
    placement = _materialize_placement_arg(placement)
    vtype = _maybe_lift_dtype_to_tensor_vtype(dtype, vtype)
    if isinstance(value, np.ndarray):
        moose_dtype = _np_to_moose_dtype(value.dtype)
        if moose_dtype is None:
            raise NotImplementedError(
                f"Tensors of dtype `{value.dtype}` not supported as graph constants."
            )
        if vtype is not None and moose_dtype != vtype.dtype:
            target = dtype or vtype.dtype
            inner = constant(value, dtype=moose_dtype, placement=placement)
            return cast(inner, target, placement)
        vtype = vtype or ty.TensorType(moose_dtype)
        return Expression("constant", placement, [], vtype,
                          {"value": values.TensorConstant(value=value)},
                          static_shape=tuple(value.shape))
    elif isinstance(value, bool):
        value = values.TensorConstant(value=np.array(value))
        vtype = vtype or ty.TensorType(dtypes.bool_)
    elif isinstance(value, (float, int)):
        if isinstance(vtype, ty.TensorType) and vtype.dtype.is_fixedpoint:
            return constant(np.array(value), vtype=vtype, placement=placement)
        fallback = ty.FloatType() if isinstance(value, float) else ty.IntType()
        value, vtype = _interpret_numeric_value(value, vtype, fallback)
    elif isinstance(value, str):
        vtype = vtype or ty.StringType()
        if not isinstance(vtype, ty.StringType):
            raise ValueError(
                f"Constant value of type `str` does not match user-supplied vtype `{vtype}`."
            )
        value = values.StringConstant(value=value)
    return Expression("constant", placement, [], vtype, {"value": value})


def _interpret_numeric_value(value, vtype, fallback_vtype):
    vtype = vtype or fallback_vtype
    if isinstance(vtype, ty.TensorType):
        d = vtype.dtype
        if not d.is_float and not d.is_integer:
            raise TypeError(f"Cannot interpret scalar constant as dtype {d}.")
        return values.TensorConstant(np.array(value, dtype=d.numpy_dtype)), vtype
    if isinstance(vtype, ty.FloatType):
        return values.FloatConstant(value), vtype
    if isinstance(vtype, ty.IntType):
        return values.IntConstant(value), vtype
    raise TypeError(f"Cannot interpret numeric constant as non-numeric type {vtype}.")


def _binary(kind, lhs, rhs, placement, vtype=None):
    assert isinstance(lhs, Expression) and isinstance(rhs, Expression)
    if vtype is None:
        vtype = _assimilate_arg_vtypes(lhs.vtype, rhs.vtype, kind)
    return _expr(kind, [lhs, rhs], vtype, placement)


def add(lhs, rhs, placement=None):
    """``lhs + rhs`` (elementwise)."""
    return _binary("add", lhs, rhs, placement)


def sub(lhs, rhs, placement=None):
    """``lhs - rhs`` (elementwise)."""
    return _binary("sub", lhs, rhs, placement)


def mul(lhs, rhs, placement=None):
    """``lhs * rhs`` (elementwise)."""
    return _binary("mul", lhs, rhs, placement)


def dot(lhs, rhs, placement=None):
    """Tensor contraction (``np.dot`` semantics for rank 1/2)."""
    return _binary("dot", lhs, rhs, placement)


def div(lhs, rhs, placement=None):
    """``lhs / rhs`` (elementwise)."""
    return _binary("div", lhs, rhs, placement)


def less(lhs, rhs, placement=None):
    """``lhs < rhs`` -> bool tensor."""
    return _binary("less", lhs, rhs, placement, vtype=ty.TensorType(dtypes.bool_))


def greater(lhs, rhs, placement=None):
    """``lhs > rhs`` -> bool tensor."""
    return _binary("greater", lhs, rhs, placement, vtype=ty.TensorType(dtypes.bool_))


def logical_and(lhs, rhs, placement=None):
    """Boolean AND."""
    return _binary("and", lhs, rhs, placement)


def logical_or(lhs, rhs, placement=None):
    """Boolean OR."""
    return _binary("or", lhs, rhs, placement)


def inverse(x, placement=None):
    """Float matrix inverse (host only)."""
    if not isinstance(x.vtype, ty.TensorType):
        raise ValueError("`inverse` operation only supports arguments of type TensorType.")
    if x.vtype.dtype not in (dtypes.float32, dtypes.float64):
        raise ValueError("`inverse` operation only supports `float32` or `float64`.")
    return _expr("inverse", [x], x.vtype, placement)


def expand_dims(x, axis, placement=None):
    """Insert singleton dimension(s) at ``axis``."""
    if isinstance(axis, int):
        axis = [axis]
    elif isinstance(axis, (tuple, list)):
        for a in axis:
            if not isinstance(a, int):
                raise ValueError(f"`axis` argument must be int or list of ints, found {type(a)}")
        axis = list(axis)
    return _expr("expand_dims", [x], x.vtype, placement, axis=axis)


def squeeze(x, axis=None, placement=None):
    """Drop singleton dimensions."""
    return _expr("squeeze", [x], x.vtype, placement, axis=axis)


def ones(shape, dtype, placement=None):
    """Tensor of ones of the given shape."""
    return _expr("ones", [_shape_operand(shape, placement)], ty.TensorType(dtype), placement)


def zeros(shape, dtype, placement=None):
    """Tensor of zeros of the given shape."""
    return _expr("zeros", [_shape_operand(shape, placement)], ty.TensorType(dtype), placement)


def square(x, placement=None):
    """``x * x``."""
    return mul(x, x, placement=placement)


def sum(x, axis=None, placement=None):
    """Sum-reduce along ``axis`` (all axes if None)."""
    return _expr("sum", [x], x.vtype, placement, axis=axis)


def mean(x, axis=None, placement=None):
    """Mean-reduce along ``axis`` (all axes if None)."""
    return _expr("mean", [x], x.vtype, placement, axis=axis)


def _unary(kind):
    def builder(x, placement=None):
        assert isinstance(x, Expression)
        return _expr(kind, [x], x.vtype, placement)

    builder.__name__ = kind
    builder.__doc__ = f"Elementwise ``{kind}``."
    return builder


exp = _unary("exp")
sqrt = _unary("sqrt")
sigmoid = _unary("sigmoid")
relu = _unary("relu")
log = _unary("log")
log2 = _unary("log2")
abs = _unary("abs")
transpose = _unary("transpose")


# ---------------------------------------------------------------------------
# piecewise-linear activations (one PiecewiseLinear operator each)
# ---------------------------------------------------------------------------
PWL_MAX = 8  # breakpoints of one PiecewiseLinear operator (MX_PWL_MAX of the native leaf)


def _pwl_dtype(fn, x):
    d = x.vtype.dtype if isinstance(x, Expression) and isinstance(x.vtype, ty.TensorType) \
        else None
    if d is None or not d.is_fixedpoint:
        raise TypeError(f"`{fn}` expects a fixed-point tensor (cast the input first), found "
                        f"{getattr(x, 'vtype', type(x).__name__)}")
    return d


def _pwl_encode(fn, what, values, frac):
    """Real numbers -> signed integers at ``frac`` fractional bits (round to nearest)."""
    out = []
    for v in values:
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating,
                                                    Fraction)):
            raise TypeError(f"`{fn}`: {what} must be real numbers, found {v!r}")
        if isinstance(v, (float, np.floating)) and not np.isfinite(v):
            raise ValueError(f"`{fn}`: {what} must be finite, found {v!r}")
        v = float(v) if isinstance(v, np.floating) else int(v) if isinstance(v, np.integer) else v
        out.append(int(round(Fraction(v) * (1 << frac))))
    return out


def _pwl_op(fn, x, breakpoints, slopes, intercepts, placement=None):
    """The PiecewiseLinear operator from integer tables at the input's fractional precision."""
    _pwl_dtype(fn, x)
    k = len(breakpoints)
    if not 1 <= k <= PWL_MAX:
        raise ValueError(f"`{fn}`: between 1 and {PWL_MAX} breakpoints, found {k}")
    if len(slopes) != k + 1 or len(intercepts) != k + 1:
        raise ValueError(f"`{fn}`: {k} breakpoints take {k + 1} slopes and intercepts, found "
                         f"{len(slopes)} and {len(intercepts)}")
    for what, vals in (("breakpoints", breakpoints), ("slopes", slopes),
                       ("intercepts", intercepts)):
        for v in vals:
            if not -(1 << 63) <= v < (1 << 63):
                raise ValueError(f"`{fn}`: {what} entry {v} (at the input's fractional "
                                 "precision) does not fit a signed 64-bit integer")
    if any(b <= a for a, b in zip(breakpoints, breakpoints[1:])):
        raise ValueError(f"`{fn}`: breakpoints must be strictly increasing at the input's "
                         f"fractional precision, found {list(breakpoints)}")
    return _expr("piecewise_linear", [x], x.vtype, placement, breakpoints=list(breakpoints),
                 slopes=list(slopes), intercepts=list(intercepts))


def piecewise_linear(x, breakpoints, slopes, intercepts, placement=None):
    """Elementwise piecewise-linear function of a fixed-point ``x`` with public pieces: ``k``
    increasing real ``breakpoints`` (at most ``PWL_MAX``) and ``k + 1`` ``slopes`` and
    ``intercepts``; the result is ``slopes[i] * x + intercepts[i]`` for ``breakpoints[i-1] <= x
    < breakpoints[i]``.  The numbers are rounded to the input's fractional precision.  On a
    secret ``x`` all ``k`` comparisons are ONE sign extraction, followed by one multiplication
    and one truncation -- the cost of a single ``relu`` whatever ``k``."""
    fn = "piecewise_linear"
    f = _pwl_dtype(fn, x).fractional_precision
    return _pwl_op(fn, x, _pwl_encode(fn, "breakpoints", breakpoints, f),
                   _pwl_encode(fn, "slopes", slopes, f),
                   _pwl_encode(fn, "intercepts", intercepts, f), placement)


def _clip(fn, x, lo, hi, placement):
    f = _pwl_dtype(fn, x).fractional_precision
    if lo is None and hi is None:
        raise ValueError(f"`{fn}` needs a lower or an upper bound")
    if lo is not None and hi is not None:
        tl, th = _pwl_encode(fn, "bounds", (lo, hi), f)
        if tl >= th:
            raise ValueError(f"`{fn}`: the lower bound {lo} is not below the upper bound {hi} "
                             "at the input's fractional precision")
        return _pwl_op(fn, x, [tl, th], [0, 1 << f, 0], [tl, 0, th], placement)
    if lo is not None:
        (tl,) = _pwl_encode(fn, "bounds", (lo,), f)
        return _pwl_op(fn, x, [tl], [0, 1 << f], [tl, 0], placement)
    (th,) = _pwl_encode(fn, "bounds", (hi,), f)
    return _pwl_op(fn, x, [th], [1 << f, 0], [0, th], placement)


def clip(x, lo=None, hi=None, placement=None):
    """``min(max(x, lo), hi)`` with public real bounds; either may be None (one-sided)."""
    return _clip("clip", x, lo, hi, placement)


def relu6(x, placement=None):
    """``min(max(x, 0), 6)``."""
    return _clip("relu6", x, 0, 6, placement)


def hard_tanh(x, min_val=-1.0, max_val=1.0, placement=None):
    """``min(max(x, min_val), max_val)``."""
    return _clip("hard_tanh", x, min_val, max_val, placement)


def leaky_relu(x, alpha=0.01, placement=None):
    """``x`` where ``x >= 0``, else ``alpha * x``."""
    fn = "leaky_relu"
    f = _pwl_dtype(fn, x).fractional_precision
    (a,) = _pwl_encode(fn, "alpha", (alpha,), f)
    return _pwl_op(fn, x, [0], [a, 1 << f], [0, 0], placement)


def _hard_sigmoid(fn, x, alpha, beta, placement):
    f = _pwl_dtype(fn, x).fractional_precision
    if not alpha > 0:
        raise ValueError(f"`{fn}`: alpha must be positive, found {alpha!r}")
    a, b = Fraction(alpha), Fraction(beta)
    t = _pwl_encode(fn, "breakpoints", (-b / a, (1 - b) / a), f)
    (ai,) = _pwl_encode(fn, "alpha", (alpha,), f)
    (bi,) = _pwl_encode(fn, "beta", (beta,), f)
    return _pwl_op(fn, x, t, [0, ai, 0], [0, bi, 1 << f], placement)


def hard_sigmoid(x, alpha=0.2, beta=0.5, placement=None):
    """``max(0, min(1, alpha * x + beta))`` (ONNX ``HardSigmoid``)."""
    return _hard_sigmoid("hard_sigmoid", x, alpha, beta, placement)


def thresholded_relu(x, alpha=1.0, placement=None):
    """``x`` where ``x > alpha``, else 0 (ONNX ``ThresholdedRelu``; discontinuous at
    ``alpha``)."""
    fn = "thresholded_relu"
    f = _pwl_dtype(fn, x).fractional_precision
    (t,) = _pwl_encode(fn, "alpha", (alpha,), f)
    # x > alpha is x >= alpha + one unit in the last place
    return _pwl_op(fn, x, [t + 1], [0, 1 << f], [0, 0], placement)


def hard_swish(x, placement=None):
    """``x * hard_sigmoid(x, 1/6, 1/2)`` (ONNX ``HardSwish``)."""
    y = mul(x, _hard_sigmoid("hard_swish", x, Fraction(1, 6), Fraction(1, 2), placement),
            placement)
    y.static_shape = x.static_shape
    return y


def tanh(x, placement=None):
    """``tanh(x) = 2 * sigmoid(2x) - 1`` on the existing sigmoid."""
    d = _pwl_dtype("tanh", x)
    s = sigmoid(add(x, x, placement), placement)
    one = constant(1.0, vtype=ty.TensorType(d), placement=placement)
    y = sub(add(s, s, placement), one, placement)
    y.static_shape = x.static_shape
    return y


# ---------------------------------------------------------------------------
# smooth activations (one PiecewisePolynomial operator each)
# ---------------------------------------------------------------------------
PWP_MAX = 8  # breakpoints of one PiecewisePolynomial operator (MX_PWP_MAX of the native leaf)
PWP_DEG = 3  # its largest degree


def _pwp_op(fn, x, breakpoints, rows, placement=None):
    """The PiecewisePolynomial operator from integer tables at the input's fractional
    precision: ``rows[j] = (c_0, .., c_d)`` of piece j."""
    _pwl_dtype(fn, x)
    k = len(breakpoints)
    if not 1 <= k <= PWP_MAX:
        raise ValueError(f"`{fn}`: between 1 and {PWP_MAX} breakpoints, found {k}")
    widths = sorted({len(r) for r in rows})
    if len(rows) != k + 1 or len(widths) != 1 or not 2 <= widths[0] <= PWP_DEG + 1:
        raise ValueError(f"`{fn}`: {k} breakpoints take {k + 1} coefficient rows of one length "
                         f"between 2 and {PWP_DEG + 1} (degree 1 to {PWP_DEG}), found "
                         f"{len(rows)} rows of lengths {widths}")
    flat = [v for r in rows for v in r]
    for what, vals in (("breakpoints", breakpoints), ("coefficients", flat)):
        for v in vals:
            if not -(1 << 63) <= v < (1 << 63):
                raise ValueError(f"`{fn}`: {what} entry {v} (at the input's fractional "
                                 "precision) does not fit a signed 64-bit integer")
    if any(b <= a for a, b in zip(breakpoints, breakpoints[1:])):
        raise ValueError(f"`{fn}`: breakpoints must be strictly increasing at the input's "
                         f"fractional precision, found {list(breakpoints)}")
    return _expr("piecewise_polynomial", [x], x.vtype, placement, breakpoints=list(breakpoints),
                 coefficients=flat, degree=widths[0] - 1)


def piecewise_polynomial(x, breakpoints, coefficients, placement=None):
    """Elementwise piecewise polynomial of a fixed-point ``x`` with public pieces: ``k``
    increasing real ``breakpoints`` (at most ``PWP_MAX``) and ``k + 1`` rows ``coefficients[j]
    = (c_0, .., c_d)`` of one degree ``d`` in 1..3; the result is ``sum_i c_i * x^i`` of row j
    for ``breakpoints[j-1] <= x < breakpoints[j]``.  The numbers are rounded to the input's
    fractional precision.  On a secret ``x`` all ``k`` comparisons are ONE sign extraction;
    the powers cost ``d - 1`` multiplications that do not wait for it, and one local kernel
    with one truncation combines them -- whatever ``k``."""
    fn = "piecewise_polynomial"
    f = _pwl_dtype(fn, x).fractional_precision
    rows = [list(r) for r in coefficients]
    return _pwp_op(fn, x, _pwl_encode(fn, "breakpoints", breakpoints, f),
                   [_pwl_encode(fn, "coefficients", r, f) for r in rows], placement)


def _smooth(fn, name, x, alpha, degree, pieces, placement):
    from moose_amd.protocols import fixedpoint as fxp

    f = _pwl_dtype(fn, x).fractional_precision
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float, np.integer, np.floating)) \
            or not np.isfinite(alpha):
        raise ValueError(f"`{fn}`: alpha must be a finite real number, found {alpha!r}")
    if name == "celu" and alpha == 0:
        raise ValueError(f"`{fn}`: alpha must not be zero")
    if degree not in (1, 2, 3):
        raise ValueError(f"`{fn}`: a degree of 1, 2 or 3, found {degree!r}")
    lo = 3 if name in ("elu", "selu", "celu") else 2
    if isinstance(pieces, bool) or not isinstance(pieces, int) or not lo <= pieces <= PWP_MAX:
        raise ValueError(f"`{fn}`: between {lo} and {PWP_MAX} breakpoints, found {pieces!r}")
    T, C, _err = fxp.smooth_tables(name, float(alpha), int(degree), pieces, f)
    return _pwp_op(fn, x, _pwl_encode(fn, "breakpoints", T, f),
                   [_pwl_encode(fn, "coefficients", r, f) for r in C], placement)


def gelu(x, approximate="none", degree=3, pieces=8, placement=None):
    """``x * Phi(x)`` (``approximate="none"``) or its tanh form (``"tanh"``) as one piecewise
    polynomial of ``degree`` with ``pieces`` breakpoints (fixedpoint.pwp_fit; the fit errors
    are listed in docs/API.md)."""
    if approximate not in ("none", "tanh"):
        raise ValueError(f"`gelu`: approximate is 'none' or 'tanh', found {approximate!r}")
    return _smooth("gelu", "gelu" if approximate == "none" else "gelu_tanh", x, 1.0, degree,
                   pieces, placement)


def silu(x, degree=3, pieces=8, placement=None):
    """``x * sigmoid(x)`` as one piecewise polynomial."""
    return _smooth("silu", "silu", x, 1.0, degree, pieces, placement)


swish = silu


def mish(x, degree=3, pieces=8, placement=None):
    """``x * tanh(softplus(x))`` as one piecewise polynomial."""
    return _smooth("mish", "mish", x, 1.0, degree, pieces, placement)


def softplus(x, degree=3, pieces=8, placement=None):
    """``log(1 + exp(x))`` as one piecewise polynomial."""
    return _smooth("softplus", "softplus", x, 1.0, degree, pieces, placement)


def elu(x, alpha=1.0, degree=3, pieces=8, placement=None):
    """``x`` where ``x > 0``, else ``alpha * (exp(x) - 1)``, as one piecewise polynomial with
    a knot at 0."""
    return _smooth("elu", "elu", x, alpha, degree, pieces, placement)


def selu(x, degree=3, pieces=8, placement=None):
    """``scale * elu(x, alpha)`` with the self-normalising constants (ONNX ``Selu``'s
    defaults)."""
    return _smooth("selu", "selu", x, 1.0, degree, pieces, placement)


def celu(x, alpha=1.0, degree=3, pieces=8, placement=None):
    """``max(0, x) + min(0, alpha * (exp(x / alpha) - 1))`` as one piecewise polynomial with
    a knot at 0."""
    return _smooth("celu", "celu", x, alpha, degree, pieces, placement)


def erf(x, degree=3, pieces=8, placement=None):
    """The error function as one piecewise polynomial (its tails are -1 and 1)."""
    return _smooth("erf", "erf", x, 1.0, degree, pieces, placement)


def softmax(x, axis, upmost_index, placement=None):
    """Softmax along ``axis`` over the first ``upmost_index`` entries."""
    return _expr("softmax", [x], x.vtype, placement, axis=axis, upmost_index=upmost_index)


def argmax(x, axis, upmost_index, placement=None):
    """Index of the maximum along ``axis``."""
    return _expr("argmax", [x], x.vtype, placement, axis=axis, upmost_index=upmost_index)


def shape(x, placement=None):
    """Shape of a tensor."""
    return _expr("shape", [x], ty.ShapeType(), placement)


def index_axis(x, axis, index, placement=None):
    """``x`` indexed at ``index`` along ``axis`` (drops the axis)."""
    if not isinstance(axis, int) or axis < 0:
        raise ValueError(f"`axis` argument must be int greater or equal to 0, found {axis}")
    if not isinstance(index, int) or index < 0:
        raise ValueError(f"`index` argument must be int greater or equal to 0, found {index}")
    return _expr("index_axis", [x], x.vtype, placement, axis=axis, index=index)


def select(x, axis, index, placement=None):
    """Keep entries along ``axis`` where the boolean ``index`` is 1."""
    if not isinstance(axis, int):
        raise ValueError(f"`axis` argument must be int, found {type(axis)}")
    return _expr("select", [x, index], x.vtype, placement, axis=axis)


def sliced(x, begin, end, placement=None):
    """``x[begin:end]`` along the first axis (tensors) or of a shape."""
    assert isinstance(begin, int) and isinstance(end, int)
    return _expr("slice", [x], x.vtype, placement, begin=begin, end=end)


def strided_slice(x, slices, placement=None):
    """General python-slice indexing."""
    for s in slices:
        if not isinstance(s, slice):
            raise ValueError(f"`slices` argument must a list/tuple of slices, found {type(s)}")
    return _expr("strided_slice", [x], x.vtype, placement, slices=list(slices))


def permute(x, axes, placement=None):
    """Reorder the axes of ``x``: result axis ``i`` is input axis ``axes[i]``."""
    if not isinstance(axes, (tuple, list)) or not all(isinstance(a, int) for a in axes):
        raise ValueError(f"`axes` argument must be a list/tuple of ints, found {axes!r}")
    axes = list(axes)
    if sorted(axes) != list(range(len(axes))):
        raise ValueError(f"`axes` argument must be a permutation of 0..{len(axes) - 1}, "
                         f"found {axes}")
    shp = x.static_shape
    if shp is not None and len(shp) != len(axes):
        raise ValueError(f"`axes` {axes} do not match a tensor of rank {len(shp)}")
    e = _expr("permute", [x], x.vtype, placement, axes=axes)
    if shp is not None:
        e.static_shape = tuple(shp[a] for a in axes)
    return e


# ---------------------------------------------------------------------------
# oblivious shuffle (one Shuffle operator each)
# ---------------------------------------------------------------------------
def _shuffle_operand(fn, x, placement):
    plc = _materialize_placement_arg(placement)
    if not isinstance(plc, ReplicatedPlacementExpression):
        raise ValueError(
            f"`{fn}` runs on a replicated placement, found {type(plc).__name__} "
            f"`{plc.name}`: a permutation drawn by one host is known to that host, so the "
            "shuffle would not be oblivious")
    d = x.vtype.dtype if isinstance(x, Expression) and isinstance(x.vtype, ty.TensorType) \
        else None
    if d is None or not d.is_fixedpoint:
        raise ValueError(f"`{fn}` expects a fixed-point tensor (cast the input first; bit "
                         f"tensors are not supported), found {getattr(x, 'vtype', type(x))}")
    return plc


def shuffle(x, axis=0, placement=None):
    """``x`` reordered along ``axis`` by a uniformly random permutation that no single party
    knows: three rounds and six messages of the tensor's size, exact -- the result holds the
    input's values in a new order, freshly re-shared.  Replicated placements and fixed-point
    tensors only.  Every evaluation draws a fresh permutation."""
    plc = _shuffle_operand("shuffle", x, placement)
    axis = _sort_axis("shuffle", axis, x.static_shape)
    e = _expr("shuffle", [x], x.vtype, plc, axis=axis)
    e.static_shape = x.static_shape
    return e


def shuffle_together(arrays, axis=0, placement=None, input_shape=None):
    """The rank-2 tensors ``arrays`` (one dtype, e.g. features and labels) shuffled by ONE
    permutation along ``axis`` 0: concatenated along axis 1, shuffled, sliced back.  The column
    widths come from each pm.Argument's ``shape=`` or from ``input_shape=``, a list with one
    shape per array."""
    fn = "shuffle_together"
    arrays = list(arrays)
    if not arrays:
        raise ValueError(f"`{fn}` takes at least one tensor")
    if axis != 0:
        raise ValueError(f"`{fn}` shuffles rows: `axis` must be 0, found {axis!r}")
    if input_shape is not None and len(input_shape) != len(arrays):
        raise ValueError(f"`{fn}`: `input_shape` must list one shape per array")
    plc = None
    widths = []
    for k, x in enumerate(arrays):
        plc = _shuffle_operand(fn, x, placement)
        shape = _sort_shape(fn, x, None if input_shape is None else input_shape[k], need=False)
        if shape is None or len(shape) != 2 or shape[1] is None:
            raise ValueError(
                f"`{fn}` needs the static column width of every rank-2 array (array {k} has "
                f"shape {shape}): pass `input_shape=`, or give the pm.Argument a `shape=`")
        widths.append(shape)
    rows = {s[0] for s in widths if s[0] is not None}
    if len(rows) > 1:
        raise ValueError(f"`{fn}`: the arrays have different numbers of rows, {sorted(rows)}")
    if len(arrays) == 1:
        return [shuffle(arrays[0], 0, plc)]
    cat = concatenate(arrays, axis=1, placement=plc)
    n = next(iter(rows), None)
    cat.static_shape = (n, builtins.sum(s[1] for s in widths))
    mixed = shuffle(cat, 0, plc)
    outs, c0 = [], 0
    for s in widths:
        y = strided_slice(mixed, [slice(None), slice(c0, c0 + s[1])], plc)
        y.static_shape = (n, s[1])
        outs.append(y)
        c0 += s[1]
    return outs


def sample_rows(x, k, placement=None):
    """``k`` rows of ``x`` drawn uniformly without replacement, in random order: a shuffle
    along axis 0 and a slice."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 0:
        raise ValueError(f"`sample_rows`: `k` must be a non-negative int, found {k!r}")
    shp = x.static_shape if isinstance(x, Expression) else None
    if shp and shp[0] is not None and shp[0] >= 0 and k > shp[0]:
        raise ValueError(f"`sample_rows`: k = {k} exceeds the {shp[0]} rows")
    s = shuffle(x, 0, placement)
    y = sliced(s, 0, int(k), s.placement)
    if shp:
        y.static_shape = (int(k),) + tuple(shp[1:])
    return y


# ---------------------------------------------------------------------------
# sorting and order statistics (one Sort operator each)
# ---------------------------------------------------------------------------
QUANTILE_INTERPOLATIONS = ("linear", "lower", "higher", "midpoint")


def _sort_shape(fn, x, input_shape, need):
    """The static shape of ``x`` (``input_shape=`` first), or None where it is unknown and not
    needed."""
    shape = tuple(input_shape) if input_shape is not None else x.static_shape
    if shape is None:
        if need:
            raise ValueError(
                f"`{fn}` needs the static length of the axis it works along: pass "
                "`input_shape=`, or give the pm.Argument a `shape=`")
        return None
    return tuple(None if s is None or s < 0 else int(s) for s in shape)


def _sort_axis(fn, axis, shape):
    if isinstance(axis, bool) or not isinstance(axis, (int, np.integer)):
        raise ValueError(f"`{fn}`: `axis` must be an int, found {axis!r}")
    axis = int(axis)
    if shape is not None:
        if not -len(shape) <= axis < len(shape):
            raise ValueError(f"`{fn}`: axis {axis} out of range for a tensor of rank {len(shape)}")
        axis %= len(shape)
    return axis


def sort(x, axis=-1, descending=False, placement=None):
    """``x`` sorted along ``axis``, ascending unless ``descending``.  On a secret fixed-point
    ``x`` a bitonic sorting network: log2 n (log2 n + 1) / 2 compare-exchange stages for an
    axis of length n (padded to a power of two), each one sign extraction and one
    multiplication; exact -- the result holds the input's values, reordered."""
    axis = _sort_axis("sort", axis, x.static_shape)
    e = _expr("sort", [x], x.vtype, placement, axis=axis, descending=bool(descending), by=-1)
    e.static_shape = x.static_shape
    return e


def sort_rows(x, by=0, descending=False, placement=None):
    """The rows of a rank-2 ``x`` reordered so that column ``by`` is sorted; rows with equal
    keys come out in unspecified order.  On a secret ``x`` the key column has to stay strictly
    inside the fixed-point type's range (a key equal to the largest encodable value may change
    places with the network's padding)."""
    if isinstance(by, bool) or not isinstance(by, (int, np.integer)) or by < 0:
        raise ValueError(f"`sort_rows`: `by` must be a column index, found {by!r}")
    shp = x.static_shape
    if shp is not None and (len(shp) != 2 or (shp[1] is not None and not by < shp[1])):
        raise ValueError(f"`sort_rows` expects a rank-2 tensor with more than {by} columns, "
                         f"found shape {shp}")
    e = _expr("sort", [x], x.vtype, placement, axis=0, descending=bool(descending), by=int(by))
    e.static_shape = shp
    return e


def _not_bits(fn, x):
    d = x.vtype.dtype if isinstance(x, Expression) and isinstance(x.vtype, ty.TensorType) \
        else None
    if d is None or d.is_boolean:
        raise ValueError(f"`{fn}` expects a float or fixed-point tensor (bit tensors are not "
                         f"supported), found {getattr(x, 'vtype', type(x))}")


def cumsum(x, axis=0, exclusive=False, reverse=False, placement=None):
    """Prefix sums of ``x`` along ``axis``: element i holds the sum of the elements up to and
    including i (``exclusive``: before i, so the first is 0; ``reverse``: counted from the far
    end).  On a host placement floats go through torch and fixed-point tensors through the
    ring scan; on a replicated placement a secret fixed-point ``x`` is summed locally on its
    shares -- no communication, exact."""
    _not_bits("cumsum", x)
    axis = _sort_axis("cumsum", axis, x.static_shape)
    e = _expr("cumsum", [x], x.vtype, placement, axis=axis, exclusive=bool(exclusive),
              reverse=bool(reverse))
    e.static_shape = x.static_shape
    return e


def group_by_sum(x, by=0, count=False, shuffle=True, placement=None, input_shape=None):
    """Group the rows of the rank-2 table ``x`` [n, c] by column ``by`` and sum every other
    column per key.  The result is [n, c + count + 1] in key order: the last row of each group
    holds the key, the column sums over the group (in the columns' order, then the group's size
    where ``count``) and ``valid = 1.0``; every other row is all zeros.

    On a replicated placement the key and the values stay secret: a sort by the key, one sign
    extraction for the group boundaries, a segmented prefix sum of ceil(log2 n)
    multiplications and one more multiplication, exact.  ``shuffle=True`` then reorders the
    rows obliviously (every evaluation draws a fresh order; such a program is not replayed).
    On a host placement the same table is computed in the clear, never shuffled.

    Limits: opening the table reveals the number of groups; without the shuffle the positions
    of the valid rows reveal the group sizes too.  ``sort_rows``' condition on the keys
    applies (strictly inside the fixed-point type's range), and the sums grow past the nominal
    integral width as those of ``mul`` and ``dot`` do.  Needs the static shape of ``x``: a
    ``shape=`` on the pm.Argument, or ``input_shape=``."""
    fn = "group_by_sum"
    _not_bits(fn, x)
    if isinstance(by, bool) or not isinstance(by, (int, np.integer)) or by < 0:
        raise ValueError(f"`{fn}`: `by` must be a column index, found {by!r}")
    shape = _sort_shape(fn, x, input_shape, need=True)
    if len(shape) != 2 or shape[1] is None or not by < shape[1]:
        raise ValueError(f"`{fn}` expects a rank-2 tensor with more than {by} columns, found "
                         f"shape {shape}")
    e = _expr("group_by_sum", [x], x.vtype, placement, by=int(by), count=bool(count),
              shuffle=bool(shuffle))
    e.static_shape = (shape[0], shape[1] + int(bool(count)) + 1)
    return e


def group_by_count(x, by=0, shuffle=True, placement=None, input_shape=None):
    """The size of every group of rows of the rank-2 ``x`` with equal values in column ``by``:
    [n, 3] in key order, the last row of each group holding (key, count, valid = 1.0), every
    other row zero -- :func:`group_by_sum` of the key column alone with ``count=True``."""
    fn = "group_by_count"
    try:
        _not_bits(fn, x)
        shape = _sort_shape(fn, x, input_shape, need=True)
        if isinstance(by, bool) or not isinstance(by, (int, np.integer)) or by < 0 \
                or len(shape) != 2 or shape[1] is None or not by < shape[1]:
            raise ValueError(f"`{fn}` expects a rank-2 tensor and a column index `by` inside "
                             f"it, found shape {shape} and by = {by!r}")
        key = strided_slice(x, [slice(None), slice(int(by), int(by) + 1)], placement)
        key.static_shape = (shape[0], 1)
        return group_by_sum(key, 0, True, shuffle, placement)
    except ValueError as e:
        raise ValueError(str(e).replace("`group_by_sum`", f"`{fn}`")) from None


def _index_arg(fn, idx):
    d = idx.vtype.dtype if isinstance(idx, Expression) and isinstance(idx.vtype, ty.TensorType) \
        else None
    if d is None or d.is_boolean:
        raise ValueError(f"`{fn}` expects a uint64 or fixed-point index tensor (bit tensors are "
                         f"not supported), found {getattr(idx, 'vtype', type(idx))}")


def _count_arg(fn, name, n):
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError(f"`{fn}`: `{name}` must be a positive integer, found {n!r}")
    return int(n)


def one_hot(idx, depth, dtype=None, placement=None):
    """The one-hot rows ``[..., depth]`` of the index tensor ``idx``: 1.0 at column ``idx`` and
    0 elsewhere, in ``dtype`` (default: the index's own type).  ``idx`` is the result of
    ``argmax`` (a uint64 tensor) or a fixed-point tensor holding integers (fractional bits are
    ignored).  On a replicated placement the index stays secret: its bits are expanded by a
    demultiplexer of ceil(log2 ceil(log2 depth)) multiplications, exact.

    Precondition: ``0 <= idx < 2^w`` with ``w = max(1, ceil(log2 depth))``; higher bits are
    ignored, and an ``idx`` in ``[depth, 2^w)`` selects nothing: its row is all zeros."""
    _index_arg("one_hot", idx)
    depth = _count_arg("one_hot", "depth", depth)
    vtype = ty.TensorType(dtype) if dtype is not None else idx.vtype
    e = _expr("one_hot", [idx], vtype, placement, depth=depth)
    if idx.static_shape is not None:
        e.static_shape = tuple(idx.static_shape) + (depth,)
    return e


def lookup(table, idx, placement=None, input_shape=None):
    """``table[idx]``: the rows of ``table`` (``[n, d]`` or ``[n]``) that the index tensor
    ``idx`` names, ``[rows, d]`` or ``[rows]`` in the table's type.  On a replicated placement
    the index stays secret and the table may be secret, mirrored or a constant: the one-hot
    matrix of the indices times the table, one untruncated ring product, so the result holds
    the table's values exactly.  Needs the table's leading size: a ``shape=`` on the
    pm.Argument, a constant, or ``input_shape=`` (the table's shape).

    Precondition: ``0 <= idx < 2^w`` with ``w = max(1, ceil(log2 n))``; higher bits are ignored,
    and an ``idx`` in ``[n, 2^w)`` selects nothing: the lookup returns 0."""
    _index_arg("lookup", idx)
    _not_bits("lookup", table)
    shape = _sort_shape("lookup", table, input_shape, need=False)
    if shape is None or len(shape) not in (1, 2) or shape[0] is None:
        raise ValueError(f"`lookup` needs a table [n, d] or [n] whose leading size is known "
                         f"(pass `input_shape=`, or give the pm.Argument a `shape=`), found "
                         f"shape {shape}")
    e = _expr("lookup", [table, idx], table.vtype, placement)
    if idx.static_shape is not None and None not in shape:
        e.static_shape = tuple(idx.static_shape) + tuple(shape[1:])
    return e


def bincount(idx, length, weights=None, placement=None):
    """The histogram of the index tensor ``idx`` over ``length`` bins: ``[length]`` counts (as
    1.0 per entry, in the index's fixed-point type), or with ``weights`` ``[rows, d]`` /
    ``[rows]`` the sums of the weights per bin, ``[length, d]`` / ``[length]`` -- a
    ``scatter_add``, the group-by of a key with a small known domain without a sort.  On a
    replicated placement: the one-hot matrix of the indices, its column sums or one
    untruncated ring product with the weights, exact.

    Precondition: ``0 <= idx < 2^w`` with ``w = max(1, ceil(log2 length))``; higher bits are
    ignored, and an ``idx`` in ``[length, 2^w)`` is counted nowhere."""
    _index_arg("bincount", idx)
    length = _count_arg("bincount", "length", length)
    if weights is not None:
        _not_bits("bincount", weights)
    e = _expr("bincount", [idx] + ([weights] if weights is not None else []),
              weights.vtype if weights is not None else idx.vtype, placement, length=length)
    if weights is None:
        e.static_shape = (length,)
    elif weights.static_shape is not None:
        e.static_shape = (length,) + tuple(weights.static_shape[1:])
    return e


def top_k(x, k, axis=-1, largest=True, placement=None, input_shape=None):
    """The ``k`` largest (``largest=False``: smallest) values along ``axis``, sorted from the
    extreme inwards: a sort and a slice.  A negative ``axis`` needs the rank of ``x`` (a
    ``shape=`` on the pm.Argument, or ``input_shape=``)."""
    fn = "top_k"
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError(f"`{fn}`: `k` must be a positive int, found {k!r}")
    shape = _sort_shape(fn, x, input_shape, need=axis < 0)
    axis = _sort_axis(fn, axis, shape)
    if shape is not None and shape[axis] is not None and k > shape[axis]:
        raise ValueError(f"`{fn}`: k = {k} exceeds the axis length {shape[axis]}")
    s = sort(x, axis, descending=bool(largest), placement=placement)
    y = strided_slice(s, [slice(None)] * axis + [slice(0, int(k))], placement)
    if shape is not None:
        y.static_shape = shape[:axis] + (int(k),) + shape[axis + 1:]
    return y


def quantile(x, q, axis=-1, interpolation="linear", placement=None, input_shape=None):
    """The ``q``-quantile (public ``q`` in [0, 1]) along ``axis``, which is dropped, as
    ``numpy.quantile``: with ``pos = q * (n - 1)`` the order statistics at ``floor(pos)`` and
    ``ceil(pos)`` are combined by ``interpolation`` -- ``lower``, ``higher``, ``midpoint`` or
    ``linear``.  ``lower`` and ``higher`` are exact; the other two cost one multiplication by a
    public weight and its truncation.  Needs the length of the axis: a ``shape=`` on the
    pm.Argument, a constant, or ``input_shape=``."""
    fn = "quantile"
    if interpolation not in QUANTILE_INTERPOLATIONS:
        raise ValueError(f"`{fn}`: interpolation must be one of {QUANTILE_INTERPOLATIONS}, found "
                         f"{interpolation!r}")
    if isinstance(q, bool) or not isinstance(q, (int, float, np.integer, np.floating)) \
            or not 0.0 <= float(q) <= 1.0:
        raise ValueError(f"`{fn}`: q must be a real number in [0, 1], found {q!r}")
    shape = _sort_shape(fn, x, input_shape, need=True)
    axis = _sort_axis(fn, axis, shape)
    n = shape[axis]
    if n is None or n < 1:
        raise ValueError(f"`{fn}` needs the static length of axis {axis}, found shape {shape}: "
                         "pass `input_shape=`, or give the pm.Argument a `shape=`")
    pos = float(q) * (n - 1)
    lo, hi = int(np.floor(pos)), int(np.ceil(pos))
    s = sort(x, axis, placement=placement)
    out_shape = shape[:axis] + shape[axis + 1:]

    def stat(i):
        e = index_axis(s, axis, i, placement)
        e.static_shape = out_shape
        return e

    if interpolation == "lower" or lo == hi:
        return stat(lo)
    if interpolation == "higher":
        return stat(hi)
    a, b = stat(lo), stat(hi)
    g = 0.5 if interpolation == "midpoint" else pos - lo
    d = x.vtype.dtype if isinstance(x.vtype, ty.TensorType) else None
    if d is not None and d.is_fixedpoint:  # the weight rounded to the nearest encodable one
        f = d.fractional_precision
        g = float(Fraction(int(round(Fraction(g) * (1 << f))), 1 << f))
    w = constant(float(g), vtype=x.vtype, placement=placement)
    y = add(a, mul(sub(b, a, placement), w, placement), placement)
    y.static_shape = out_shape
    return y


def median(x, axis=-1, placement=None, input_shape=None):
    """The median along ``axis`` (dropped): the middle order statistic of an odd length,
    exact; the mean of the two middle ones of an even length."""
    try:
        return quantile(x, 0.5, axis, "linear", placement, input_shape)
    except ValueError as e:
        raise ValueError(str(e).replace("`quantile`", "`median`")) from None


def _conv_geometry(fn, shape, kernel_shape, strides, pads, dilations, data_format):
    """Validated attributes of a 2-D window op, and (C, H, W, OH, OW) where the static
    ``shape`` (rank 4, batch entry may be None) is known."""
    if data_format not in ("NCHW", "NHWC"):
        raise ValueError(f"`{fn}`: data_format must be 'NCHW' or 'NHWC', found {data_format!r}")
    for name, v, n in (("kernel_shape", kernel_shape, 2), ("strides", strides, 2),
                       ("pads", pads, 4), ("dilations", dilations, 2)):
        if not isinstance(v, (tuple, list)) or len(v) != n or \
                not all(isinstance(i, int) for i in v):
            raise ValueError(f"`{fn}`: `{name}` must be a list/tuple of {n} ints, found {v!r}")
    if builtins.min(kernel_shape) <= 0:
        raise ValueError(f"`{fn}`: kernel_shape must be positive, found {tuple(kernel_shape)}")
    if builtins.min(strides) <= 0 or builtins.min(dilations) <= 0:
        raise ValueError(f"`{fn}`: strides and dilations must be positive, found "
                         f"{tuple(strides)} and {tuple(dilations)}")
    if builtins.min(pads) < 0:
        raise ValueError(f"`{fn}`: pads must be non-negative, found {tuple(pads)}")
    if shape is None:
        return None
    if len(shape) != 4:
        raise ValueError(f"`{fn}` expects a rank-4 {data_format} tensor, found shape "
                         f"{tuple(shape)}")
    c, h, w = (shape[1:] if data_format == "NCHW" else (shape[3], shape[1], shape[2]))
    if None in (c, h, w):
        return None
    (kh, kw), (sh, sw), (pt, pl, pb, pr), (dh, dw) = kernel_shape, strides, pads, dilations
    oh = (h + pt + pb - dh * (kh - 1) - 1) // sh + 1
    ow = (w + pl + pr - dw * (kw - 1) - 1) // sw + 1
    if oh <= 0 or ow <= 0:
        raise ValueError(f"`{fn}`: a {kh}x{kw} kernel does not fit the padded "
                         f"{h + pt + pb}x{w + pl + pr} image (output {oh}x{ow})")
    return c, h, w, oh, ow


def im2col(x, kernel_shape, strides=(1, 1), pads=(0, 0, 0, 0), dilations=(1, 1),
           data_format="NCHW", placement=None, input_shape=None):
    """Patch matrix ``[N*OH*OW, C*KH*KW]`` of a rank-4 tensor: rows ordered (n, oh, ow),
    columns (c, kh, kw) for NCHW and (kh, kw, c) for NHWC; ``pads`` is (top, left, bottom,
    right) and padded taps are zero.  ``input_shape`` is the static shape of ``x`` where the
    expression does not carry it (optional: it only types the result)."""
    shape = tuple(input_shape) if input_shape is not None else x.static_shape
    g = _conv_geometry("im2col", shape, kernel_shape, strides, pads, dilations, data_format)
    e = _expr("im2col", [x], x.vtype, placement, kernel_shape=list(kernel_shape),
              strides=list(strides), pads=list(pads), dilations=list(dilations),
              data_format=data_format)
    if g is not None:
        c, _h, _w, oh, ow = g
        n = shape[0]
        e.static_shape = (None if n is None or n < 0 else n * oh * ow,
                          c * kernel_shape[0] * kernel_shape[1])
    return e


def _window_input(fn, x, input_shape, data_format):
    shape = tuple(input_shape) if input_shape is not None else x.static_shape
    if shape is None:
        raise ValueError(
            f"`{fn}` needs the static shape of its input (the batch size may be None): "
            "pass `input_shape=`, or give the pm.Argument a `shape=`")
    shape = tuple(None if s is None or s < 0 else int(s) for s in shape)
    if len(shape) != 4:
        raise ValueError(f"`{fn}` expects a rank-4 {data_format} tensor, found shape {shape}")
    if None in shape[1:]:
        raise ValueError(f"`{fn}`: only the batch size may be unknown, found shape {shape}")
    return shape


def _batch(n):
    return -1 if n is None else n


def _weight_shape(fn, w, weight_shape, layout):
    ws = tuple(weight_shape) if weight_shape is not None else w.static_shape
    if ws is None:
        raise ValueError(f"`{fn}` needs the static shape of `w`: pass `weight_shape=`")
    if len(ws) != 4 or None in ws:
        raise ValueError(f"`{fn}` expects `w` of shape {layout}, found {tuple(ws)}")
    return tuple(int(s) for s in ws)


def _channel_bias(bias, oc, data_format, placement):
    """``bias`` ([OC]) shaped to broadcast over a rank-4 activation in ``data_format``."""
    return bias if data_format == "NHWC" else reshape(bias, [oc, 1, 1], placement)


def depthwise_conv2d(x, w, bias=None, strides=(1, 1), pads=(0, 0, 0, 0), dilations=(1, 1),
                     data_format="NCHW", placement=None, input_shape=None, weight_shape=None):
    """Depthwise 2-D convolution (ONNX ``Conv`` with ``group = C``) of ``x`` (rank 4,
    ``data_format``) with ``w`` of shape ``[C*mult, 1, KH, KW]``: output channel ``c*mult + j``
    is input channel ``c`` filtered by ``w[c*mult + j, 0]`` (+ ``bias`` of shape ``[C*mult]``).
    One ``DepthwiseConv`` operator -- a direct stencil over the shares, no patch matrix; the
    result keeps the input's ``data_format`` and carries a static shape.  Static shapes as
    :func:`conv2d`."""
    if data_format not in ("NCHW", "NHWC"):
        raise ValueError(f"`depthwise_conv2d`: data_format must be 'NCHW' or 'NHWC', found "
                         f"{data_format!r}")
    oc, w1, kh, kw = _weight_shape("depthwise_conv2d", w, weight_shape, "[C*mult, 1, KH, KW]")
    xs = _window_input("depthwise_conv2d", x, input_shape, data_format)
    c, _h, _w, oh, ow = _conv_geometry("depthwise_conv2d", xs, (kh, kw), strides, pads,
                                       dilations, data_format)
    if w1 != 1:
        raise ValueError(f"`depthwise_conv2d` expects `w` of shape [C*mult, 1, KH, KW], found "
                         f"{(oc, w1, kh, kw)} (w.shape[1] = {w1})")
    if oc % c:
        raise ValueError(f"`depthwise_conv2d`: `w` has {oc} output channels, not a multiple of "
                         f"the input's {c} channels")
    y = _expr("depthwise_conv", [x, w], x.vtype, placement, strides=list(strides),
              pads=list(pads), dilations=list(dilations), data_format=data_format)
    y.static_shape = (xs[0], oc, oh, ow) if data_format == "NCHW" else (xs[0], oh, ow, oc)
    if bias is not None:
        static = y.static_shape
        y = add(y, _channel_bias(bias, oc, data_format, placement), placement)
        y.static_shape = static
    return y


def conv2d(x, w, bias=None, strides=(1, 1), pads=(0, 0, 0, 0), dilations=(1, 1),
           data_format="NCHW", placement=None, input_shape=None, weight_shape=None, groups=1):
    """2-D convolution (cross-correlation, as ONNX ``Conv``) of ``x`` (rank 4, ``data_format``)
    with ``w`` of shape ``[OC, C // groups, KH, KW]`` (+ ``bias`` of shape ``[OC]``); the result
    has the input's ``data_format``.  ``groups = 1``: ``im2col`` + one ``dot``.  ``groups = C``:
    the depthwise operator (:func:`depthwise_conv2d`).  ``1 < groups < C``: a composition --
    a channel slice of ``x`` and of ``w`` per group, ``im2col`` + ``dot`` on each, and
    ``concatenate`` on the channel axis: ``groups`` products, not a fast path.  The static
    shapes come from the expressions (constants, ``pm.Argument(shape=...)``) or from
    ``input_shape`` / ``weight_shape``; only the batch size may be unknown (None)."""
    if data_format not in ("NCHW", "NHWC"):
        raise ValueError(f"`conv2d`: data_format must be 'NCHW' or 'NHWC', found {data_format!r}")
    if not isinstance(groups, int) or isinstance(groups, bool) or groups < 1:
        raise ValueError(f"`conv2d`: groups must be a positive int, found {groups!r}")
    ws = _weight_shape("conv2d", w, weight_shape, "[OC, C, KH, KW] (C // groups with groups)")
    oc, wc, kh, kw = ws
    xs = _window_input("conv2d", x, input_shape, data_format)
    c, _h, _w, oh, ow = _conv_geometry("conv2d", xs, (kh, kw), strides, pads, dilations,
                                       data_format)
    if groups > 1:
        if c % groups:
            raise ValueError(f"`conv2d`: groups = {groups} does not divide the input's {c} "
                             "channels")
        if oc % groups:
            raise ValueError(f"`conv2d`: groups = {groups} does not divide the {oc} output "
                             f"channels of `w` {ws}")
    if c != wc * groups:
        raise ValueError(f"`conv2d`: input has {c} channels and groups = {groups}, so `w` "
                         f"must have {c // groups} input channels per group, but `w` {ws} has "
                         f"{wc}")
    if groups > 1 and groups == c:
        return depthwise_conv2d(x, w, bias, strides, pads, dilations, data_format, placement,
                                xs, ws)
    if groups > 1:
        cg, ocg = c // groups, oc // groups
        cax = 1 if data_format == "NCHW" else 3
        gshape = tuple(cg if i == cax else s for i, s in enumerate(xs))
        parts = []
        for g in range(groups):
            sl = [slice(None)] * 4
            sl[cax] = slice(g * cg, (g + 1) * cg)
            xg = strided_slice(x, sl, placement)
            wg = strided_slice(w, [slice(g * ocg, (g + 1) * ocg)] + [slice(None)] * 3, placement)
            parts.append(conv2d(xg, wg, None, strides, pads, dilations, data_format, placement,
                                gshape, (ocg, cg, kh, kw)))
        y = concatenate(parts, axis=cax, placement=placement)
        if bias is not None:
            y = add(y, _channel_bias(bias, oc, data_format, placement), placement)
        y.static_shape = (xs[0], oc, oh, ow) if data_format == "NCHW" else (xs[0], oh, ow, oc)
        return y
    k = c * kh * kw
    cols = im2col(x, (kh, kw), strides, pads, dilations, data_format, placement, xs)
    if data_format == "NCHW":
        wm = transpose(reshape(w, [oc, k], placement), placement)
    else:  # rows in the patch matrix's (kh, kw, c) order
        wm = reshape(permute(w, (2, 3, 1, 0), placement), [k, oc], placement)
    y = dot(cols, wm, placement)
    if bias is not None:
        y = add(y, bias, placement)
    y = reshape(y, [_batch(xs[0]), oh, ow, oc], placement)
    y.static_shape = (xs[0], oh, ow, oc)
    if data_format == "NCHW":
        y = permute(y, (0, 3, 1, 2), placement)
    return y


def col2im(cols, image_shape, kernel_shape, strides=(1, 1), pads=(0, 0, 0, 0),
           dilations=(1, 1), data_format="NCHW", placement=None):
    """The exact adjoint of :func:`im2col`: the patch matrix ``cols`` (``[N*OH*OW, C*KH*KW]``,
    im2col's row and column order) summed into the image ``[N, C, H, W]`` (NHWC: ``[N, H, W,
    C]``) of ``image_shape = (C, H, W)``: every pixel is the sum of the entries whose tap lands
    on it, entries in the padding are dropped and a pixel no window reaches is zero.  The
    batch size comes from the rows."""
    if not isinstance(image_shape, (tuple, list)) or len(image_shape) != 3 or \
            not all(isinstance(i, int) and i > 0 for i in image_shape):
        raise ValueError("`col2im`: `image_shape` must be 3 positive ints (C, H, W), found "
                         f"{image_shape!r}")
    c, h, w = image_shape
    shape = (None, c, h, w) if data_format != "NHWC" else (None, h, w, c)
    _c, _h, _w, oh, ow = _conv_geometry("col2im", shape, kernel_shape, strides, pads, dilations,
                                        data_format)
    n = None
    cs = cols.static_shape
    if cs is not None:
        k = c * kernel_shape[0] * kernel_shape[1]
        if len(cs) != 2 or (cs[1] is not None and cs[1] != k):
            raise ValueError(f"`col2im` expects a patch matrix [N*{oh * ow}, {k}], found shape "
                             f"{tuple(cs)}")
        if cs[0] is not None and cs[0] >= 0:
            if cs[0] % (oh * ow):
                raise ValueError(f"`col2im`: {cs[0]} rows are not a multiple of the {oh}x{ow} "
                                 f"windows of a {h}x{w} image")
            n = cs[0] // (oh * ow)
    e = _expr("col2im", [cols], cols.vtype, placement, image_shape=list(image_shape),
              kernel_shape=list(kernel_shape), strides=list(strides), pads=list(pads),
              dilations=list(dilations), data_format=data_format)
    e.static_shape = (n, c, h, w) if data_format == "NCHW" else (n, h, w, c)
    return e


def conv_transpose2d(x, w, bias=None, strides=(1, 1), pads=(0, 0, 0, 0), dilations=(1, 1),
                     output_padding=(0, 0), data_format="NCHW", placement=None,
                     input_shape=None, weight_shape=None):
    """Transposed 2-D convolution (ONNX ``ConvTranspose``, ``group = 1``) of ``x`` (rank 4,
    ``data_format``) with ``w`` of shape ``[C, OC, KH, KW]`` (+ ``bias`` of shape ``[OC]``); the
    result has the input's ``data_format`` and the spatial size ``(H - 1)*sh + dh*(KH - 1) + 1
    - pt - pb + output_padding[0]`` (width alike).  One ``dot`` of the pixels with the weight,
    then :func:`col2im` -- the adjoint of the patch gather, a sum over shares -- into the
    output image: the forward geometry of that image with the same attributes is exactly
    ``H x W`` while ``output_padding < strides``.  Static shapes as :func:`conv2d`."""
    if data_format not in ("NCHW", "NHWC"):
        raise ValueError("`conv_transpose2d`: data_format must be 'NCHW' or 'NHWC', found "
                         f"{data_format!r}")
    wc, oc, kh, kw = _weight_shape("conv_transpose2d", w, weight_shape, "[C, OC, KH, KW]")
    xs = _window_input("conv_transpose2d", x, input_shape, data_format)
    _conv_geometry("conv_transpose2d", None, (kh, kw), strides, pads, dilations, data_format)
    if not isinstance(output_padding, (tuple, list)) or len(output_padding) != 2 or \
            not all(isinstance(i, int) for i in output_padding):
        raise ValueError("`conv_transpose2d`: `output_padding` must be a list/tuple of 2 ints, "
                         f"found {output_padding!r}")
    if not all(0 <= o < s for o, s in zip(output_padding, strides)):
        raise ValueError("`conv_transpose2d`: output_padding must be non-negative and below "
                         f"the strides, found {tuple(output_padding)} with strides "
                         f"{tuple(strides)}")
    c, h, wd = (xs[1:] if data_format == "NCHW" else (xs[3], xs[1], xs[2]))
    if c != wc:
        raise ValueError(f"`conv_transpose2d`: input has {c} channels, but `w` "
                         f"{(wc, oc, kh, kw)} expects {wc} (w.shape[0])")
    (sh, sw), (pt, pl, pb, pr), (dh, dw) = strides, pads, dilations
    oht = (h - 1) * sh + dh * (kh - 1) + 1 - pt - pb + output_padding[0]
    owt = (wd - 1) * sw + dw * (kw - 1) + 1 - pl - pr + output_padding[1]
    if oht <= 0 or owt <= 0:
        raise ValueError(f"`conv_transpose2d`: pads {tuple(pads)} leave no output "
                         f"({oht}x{owt})")
    if data_format == "NCHW":
        xr = reshape(permute(x, (0, 2, 3, 1), placement), [-1, c], placement)
        wm = reshape(w, [c, oc * kh * kw], placement)
    else:  # columns in the patch matrix's (kh, kw, oc) order
        xr = reshape(x, [-1, c], placement)
        wm = reshape(permute(w, (0, 2, 3, 1), placement), [c, kh * kw * oc], placement)
    cols = dot(xr, wm, placement)
    y = col2im(cols, (oc, oht, owt), (kh, kw), strides, pads, dilations, data_format, placement)
    static = (xs[0], oc, oht, owt) if data_format == "NCHW" else (xs[0], oht, owt, oc)
    y.static_shape = static
    if bias is not None:
        y = add(y, _channel_bias(bias, oc, data_format, placement), placement)
        y.static_shape = static
    return y


def resize2d(x, sizes=None, scales=None, mode="nearest",
             coordinate_transformation_mode="half_pixel", nearest_mode="round_prefer_floor",
             data_format="NCHW", weight_bits=None, placement=None, input_shape=None):
    """Resize the spatial axes of ``x`` (rank 4, ``data_format``) as ONNX ``Resize`` does, in
    ``nearest`` or (bi)``linear`` mode.  Exactly one of ``sizes = (OH, OW)`` and ``scales =
    (scale_h, scale_w)`` is given; with ``scales`` the output size is ``floor(I * scale)`` and
    the coordinates use the given scale.  The coordinates are public, so on a replicated
    placement the operator is local on the shares; ``linear`` on fixed point multiplies by
    integer weights of ``weight_bits = (wbh, wbw)`` bits per axis and truncates once by ``wbh
    + wbw``.  The default ``weight_bits`` is, per axis, the smallest width in 0..12 at which
    every weight is exact (2x ``half_pixel``: 2; an axis that keeps its size: 0), else 12: an
    inexact weight is off by at most ``2^-(wb + 1)``.  Static shapes as :func:`conv2d`."""
    from moose_amd.ops import ring as R

    fn = "resize2d"
    if data_format not in ("NCHW", "NHWC"):
        raise ValueError(f"`{fn}`: data_format must be 'NCHW' or 'NHWC', found {data_format!r}")
    if mode not in R.RESIZE_MODES:
        raise ValueError(f"`{fn}`: `mode` must be one of {R.RESIZE_MODES}, found {mode!r}")
    if coordinate_transformation_mode not in R.RESIZE_COORDS:
        raise ValueError(f"`{fn}`: `coordinate_transformation_mode` must be one of "
                         f"{R.RESIZE_COORDS}, found {coordinate_transformation_mode!r}")
    if nearest_mode not in R.RESIZE_NEAREST:
        raise ValueError(f"`{fn}`: `nearest_mode` must be one of {R.RESIZE_NEAREST}, found "
                         f"{nearest_mode!r}")
    if (sizes is None) == (scales is None):
        raise ValueError(f"`{fn}`: exactly one of `sizes` and `scales` must be given, found "
                         f"sizes={sizes!r} and scales={scales!r}")
    xs = _window_input(fn, x, input_shape, data_format)
    h, w = (xs[2], xs[3]) if data_format == "NCHW" else (xs[1], xs[2])
    fracs = (None, None)
    if sizes is not None:
        if not isinstance(sizes, (tuple, list)) or len(sizes) != 2 or \
                not all(isinstance(i, int) and not isinstance(i, bool) for i in sizes):
            raise ValueError(f"`{fn}`: `sizes` must be a list/tuple of 2 ints (OH, OW), found "
                             f"{sizes!r}")
        if builtins.min(sizes) <= 0:
            raise ValueError(f"`{fn}`: `sizes` must be positive, found {tuple(sizes)}")
        oh, ow = sizes
    else:
        if not isinstance(scales, (tuple, list)) or len(scales) != 2 or \
                not all(isinstance(s, (int, float)) and not isinstance(s, bool)
                        for s in scales):
            raise ValueError(f"`{fn}`: `scales` must be a list/tuple of 2 numbers (scale_h, "
                             f"scale_w), found {scales!r}")
        if not all(s > 0 and s == s and s != float("inf") for s in scales):
            raise ValueError(f"`{fn}`: `scales` must be positive and finite, found "
                             f"{tuple(scales)}")
        fracs = tuple(R.resize_scale(s) for s in scales)
        oh, ow = (int(i * s) for i, s in zip((h, w), fracs))  # floor of the exact product
        if oh <= 0 or ow <= 0:
            raise ValueError(f"`{fn}`: `scales` {tuple(scales)} leave no output ({oh}x{ow}) of "
                             f"a {h}x{w} image")
        if builtins.max(f.numerator.bit_length() for f in fracs) > 62 or \
                builtins.max(f.denominator.bit_length() for f in fracs) > 62:
            raise ValueError(f"`{fn}`: `scales` {tuple(scales)} are not representable as "
                             "ratios of 62-bit integers")
    axes = ((h, oh, fracs[0]), (w, ow, fracs[1]))
    if weight_bits is None:
        weight_bits = tuple(R.resize_weight_bits(i, o, mode, coordinate_transformation_mode,
                                                 nearest_mode, s) for i, o, s in axes)
    elif not isinstance(weight_bits, (tuple, list)) or len(weight_bits) != 2 or \
            not all(isinstance(b, int) and not isinstance(b, bool) and
                    0 <= b <= R.RESIZE_MAX_WEIGHT_BITS for b in weight_bits):
        raise ValueError(f"`{fn}`: `weight_bits` must be 2 ints in 0.."
                         f"{R.RESIZE_MAX_WEIGHT_BITS} (height, width), found {weight_bits!r}")
    if mode == "nearest":
        weight_bits = (0, 0)
    dtype = x.vtype.dtype if isinstance(x.vtype, ty.TensorType) else None
    wb = builtins.sum(weight_bits)
    if wb and dtype is not None and dtype.is_fixedpoint:
        # the truncation protocol is valid for |x| < 2^(k - 2); an unpinned dtype is checked
        # against the widest ring here and against the run's ring when it is evaluated
        ring = dtype.ring or 128
        need = dtype.integral_precision + dtype.fractional_precision + wb
        if need > ring - 2:
            raise ValueError(
                f"`{fn}`: {dtype.integral_precision} integral + {dtype.fractional_precision} "
                f"fractional + {wb} weight bits = {need} exceed the {ring - 2} bits a "
                f"truncation in Z_2^{ring} can take: pass a smaller `weight_bits`")
    if wb and dtype is not None and dtype.is_boolean:
        raise ValueError(f"`{fn}`: `mode` 'linear' on a bool tensor: a weighted sum of bits is "
                         "not a bit")
    sc = [] if scales is None else [fracs[0].numerator, fracs[0].denominator,
                                    fracs[1].numerator, fracs[1].denominator]
    e = _expr("resize", [x], x.vtype, placement, sizes=[oh, ow], mode=mode,
              coordinate_transformation_mode=coordinate_transformation_mode,
              nearest_mode=nearest_mode, scales=sc, weight_bits=list(weight_bits),
              data_format=data_format)
    e.static_shape = (xs[0], xs[1], oh, ow) if data_format == "NCHW" else (xs[0], oh, ow, xs[3])
    return e


def _pool_taps(fn, x, kernel_shape, strides, pads, data_format, placement, input_shape):
    """([M, KH*KW] or [M, KH*KW, C] tap matrix, tap axis, result builder) of a pooling."""
    strides = tuple(kernel_shape) if strides is None else strides
    xs = _window_input(fn, x, input_shape, data_format)
    c, h, w, oh, ow = _conv_geometry(fn, xs, kernel_shape, strides, pads, (1, 1), data_format)
    taps = kernel_shape[0] * kernel_shape[1]
    if data_format == "NCHW":
        # every channel is an image of its own: no permute on shares
        per = reshape(x, [-1, 1, h, w], placement)
        per.static_shape = (None, 1, h, w)
        cols = im2col(per, kernel_shape, strides, pads, (1, 1), "NCHW", placement)
        out = [_batch(xs[0]), c, oh, ow]
        static = (xs[0], c, oh, ow)
    else:
        cols = im2col(x, kernel_shape, strides, pads, (1, 1), "NHWC", placement, xs)
        cols = reshape(cols, [-1, taps, c], placement)
        out = [_batch(xs[0]), oh, ow, c]
        static = (xs[0], oh, ow, c)

    def finish(y):
        y = reshape(y, out, placement)
        y.static_shape = static
        return y

    return cols, taps, finish


def avg_pool2d(x, kernel_shape, strides=None, pads=(0, 0, 0, 0), data_format="NCHW",
               placement=None, input_shape=None):
    """2-D average pooling (``strides`` default to ``kernel_shape``): ``im2col`` on a
    per-channel view, then ``mean`` over the taps.  Padded taps count as zeros (ONNX
    ``count_include_pad=1``)."""
    cols, _taps, finish = _pool_taps("avg_pool2d", x, kernel_shape, strides, pads, data_format,
                                     placement, input_shape)
    return finish(mean(cols, axis=1, placement=placement))


def max_pool2d(x, kernel_shape, strides=None, data_format="NCHW", placement=None,
               input_shape=None):
    """2-D max pooling without padding: ``im2col``, one ``index_axis`` per tap, then
    ``maximum``."""
    cols, taps, finish = _pool_taps("max_pool2d", x, kernel_shape, strides, (0, 0, 0, 0),
                                    data_format, placement, input_shape)
    views = [index_axis(cols, axis=1, index=t, placement=placement) for t in range(taps)]
    return finish(views[0] if taps == 1 else maximum(views, placement))


def atleast_2d(x, to_column_vector=False, placement=None):
    """Promote rank<2 tensors to rank 2."""
    return _expr("atleast_2d", [x], x.vtype, placement, to_column_vector=to_column_vector)


def reshape(x, shape, placement=None):
    """Reshape ``x`` to ``shape`` (list/tuple or Shape expression)."""
    return _expr("reshape", [x, _shape_operand(shape, placement)], x.vtype, placement)


def mux(selector, x, y, placement=None):
    """``selector ? x : y`` on a replicated placement."""
    assert isinstance(selector.vtype, ty.TensorType) and selector.vtype.dtype.is_boolean
    assert isinstance(x.vtype, ty.TensorType) and x.vtype.dtype.is_fixedpoint
    assert isinstance(y.vtype, ty.TensorType) and y.vtype.dtype.is_fixedpoint
    plc = _materialize_placement_arg(placement)
    assert isinstance(plc, ReplicatedPlacementExpression)
    vt = _assimilate_arg_vtypes(x.vtype, y.vtype, "mux")
    return _expr("mux", [selector, x, y], vt, plc)


def cast(x, dtype, placement=None):
    """Convert a tensor to ``dtype`` (float<->fixed encode/decode, int casts...)."""
    if not isinstance(x.vtype, ty.TensorType):
        raise ValueError(f"Argument to `cast` operation must be tensor, found {x.vtype}.")
    if x.vtype.dtype is None:
        raise ValueError("Argument to `cast` function must have well-defined dtype.")
    if dtype is None:
        raise ValueError("Invalid `dtype` argument to `cast` function: cannot cast to None.")
    if isinstance(dtype, dtypes.DType):
        target = dtype
    else:
        target = _np_to_moose_dtype(dtype)
        if target is None:
            raise ValueError(f"Unsupported dtype arg in `cast` function: {dtype}.")
    if x.vtype.dtype == target:
        return x
    return _expr("cast", [x], ty.TensorType(target), placement)


def _string_operand(v, placement, fn, what):
    if isinstance(v, str):
        return constant(v, placement=placement, vtype=ty.StringType())
    if isinstance(v, Argument) and v.vtype not in (ty.StringType(), None):
        raise ValueError(f"Function 'edsl.{fn}' encountered `{what}` of vtype {v.vtype}.")
    if not isinstance(v, Expression):
        raise ValueError(f"Function 'edsl.{fn}' encountered `{what}` of type {type(v)}.")
    return v


def load(key, query="", dtype=None, vtype=None, placement=None):
    """Load a value from the placement's storage."""
    placement = _materialize_placement_arg(placement)
    vtype = _maybe_lift_dtype_to_tensor_vtype(dtype, vtype)
    key = _string_operand(key, placement, "load", "key")
    query = _string_operand(query, placement, "load", "query")
    return _expr("load", [key, query], vtype, placement)


def save(key, value, placement=None):
    """Save ``value`` under ``key`` in the placement's storage."""
    assert isinstance(value, Expression)
    placement = _materialize_placement_arg(placement)
    key = _string_operand(key, placement, "save", "key")
    return _expr("save", [key, value], None, placement)


def output(tag, value, placement=None):
    """Tag an output of the computation."""
    assert isinstance(value, Expression) and isinstance(tag, str)
    return _expr("output", [value], value.vtype, placement, tag=tag)


# ---------------------------------------------------------------------------
# computations
# ---------------------------------------------------------------------------
def computation(func=None, role_map=None):
    """Decorate a python function as an (abstract) Moose computation."""
    if func is None:
        return ft.partial(computation, role_map=role_map)
    return AbstractComputation(func, role_map)


class AbstractComputation:
    def __init__(self, func, role_map):
        if not callable(func):
            raise TypeError(f"Argument `func` should be a callable, but found {type(func)}.")
        if role_map is not None and not isinstance(role_map, dict):
            raise TypeError(
                f"Argument `role_map` should be map of placement names, found {type(role_map)}."
            )
        self.func = func
        self.role_map = role_map

    def __call__(self, *args, **kwargs):
        names = list(inspect.signature(self.func).parameters)
        if len(args) > len(names):
            raise ValueError(f"Too many arguments for `{self.func.__name__}`")
        arguments = dict(zip(names, args))
        for k, v in kwargs.items():
            if k in arguments:
                raise ValueError(f"Argument `{k}` given more than once to `{self.func.__name__}`")
            if k not in names:
                raise ValueError(f"Argument `{k}` is not used by `{self.func.__name__}`")
            arguments[k] = v
        for n in names:
            if n not in arguments:
                raise ValueError(f"Missing argument `{n}` in call to `{self.func.__name__}`")
        runtime = get_current_runtime()
        if not runtime:
            raise RuntimeError("No default runtime found")
        return runtime.evaluate_computation(self, arguments)

    def with_role_map(self, role_map):
        return self.__class__(self.func, role_map)


__all__ = [n for n in dir() if not n.startswith("_") and n not in ("builtins",)]
