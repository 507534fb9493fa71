"""pm.sort, pm.sort_rows, pm.top_k, pm.median and pm.quantile through LocalMooseRuntime: exact
against numpy on the decoded inputs (a sort truncates nothing), replayed, with the parties as
threads, lowered to a graph without an operator of its own, serialised, and on a host."""
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
DEVICES = ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)]
XS, TS = (4, 7), (6, 3)  # an odd axis of 7 (padded to 8), an even one of 4; a table of 6 rows
Q = 0.3

# name -> (builder on (x, t), numpy on (x, t)); all of these are exact
EXACT = {
    "sort": (lambda x, t: pm.sort(x), lambda x, t: np.sort(x, axis=-1)),
    "sort_axis0_desc": (lambda x, t: pm.sort(x, axis=0, descending=True),
                        lambda x, t: -np.sort(-x, axis=0)),
    "sort_rows": (lambda x, t: pm.sort_rows(t, by=1), lambda x, t: t[np.argsort(t[:, 1])]),
    "sort_rows_desc": (lambda x, t: pm.sort_rows(t, by=0, descending=True),
                       lambda x, t: t[np.argsort(-t[:, 0])]),
    "top_k": (lambda x, t: pm.top_k(x, 3), lambda x, t: -np.sort(-x, axis=-1)[:, :3]),
    "bottom_k": (lambda x, t: pm.top_k(x, 2, axis=0, largest=False),
                 lambda x, t: np.sort(x, axis=0)[:2]),
    "median_odd": (lambda x, t: pm.median(x), lambda x, t: np.median(x, axis=-1)),
    "q_lower": (lambda x, t: pm.quantile(x, Q, interpolation="lower"),
                lambda x, t: np.quantile(x, Q, axis=-1, method="lower")),
    "q_higher": (lambda x, t: pm.quantile(x, Q, axis=0, interpolation="higher"),
                 lambda x, t: np.quantile(x, Q, axis=0, method="higher")),
}
# name -> (builder, numpy, axis): one multiplication by a public weight and its truncation
INTERPOLATED = {
    "q_midpoint": (lambda x, t: pm.quantile(x, Q, interpolation="midpoint"),
                   lambda x, t: np.quantile(x, Q, axis=-1, method="midpoint"), -1),
    "q_linear": (lambda x, t: pm.quantile(x, Q, interpolation="linear"),
                 lambda x, t: np.quantile(x, Q, axis=-1, method="linear"), -1),
    "median_even": (lambda x, t: pm.median(x, axis=0), lambda x, t: np.median(x, axis=0), 0),
}
NAMES = list(EXACT) + list(INTERPOLATED)


def _inputs(f):
    """x and a table t on the 2^-f grid (the decoded inputs are the inputs): duplicates and
    negatives in x, distinct keys in the columns of t."""
    rng = np.random.default_rng(3)
    grid = lambda a: np.round(a * 2.0 ** f) / 2.0 ** f  # noqa: E731
    x = grid(rng.uniform(-50, 50, XS))
    x[0, 1], x[2, 5] = x[0, 4], x[2, 0]
    t = grid(rng.uniform(-50, 50, TS))
    t[:, 0] = rng.permutation(TS[0]) - 2.5
    t[:, 1] = (rng.permutation(TS[0]) - 3) * 0.75
    return x, t


def _program(ring, names=NAMES, shapes=True):
    dt = DTYPES[ring]
    fns = {**EXACT, **INTERPOLATED}
    kx = {"shape": XS} if shapes else {}
    kt = {"shape": TS} if shapes else {}

    @pm.computation
    def prog(x: pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64), **kx),
             t: pm.Argument(placement=BOB, vtype=pm.TensorType(pm.float64), **kt)):
        with ALICE:
            xf = pm.cast(x, dtype=dt)
        with BOB:
            tf = pm.cast(t, dtype=dt)
        with REP:
            ys = [fns[n][0](xf, tf) for n in names]
        with CAROLE:
            return tuple(pm.cast(y, dtype=pm.float64) for y in ys)

    return prog


_RUNS = {}


def _evaluate_thrice(device, ring):
    """Three evaluations of one program: on a device the second and third replay its graph."""
    key = (device, ring)
    if key not in _RUNS:
        x, t = _inputs(FRAC[ring])
        kw = {"use_graphs": True} if device != "cpu" else {}
        rt = LocalMooseRuntime(ROLES, device=device, fixedpoint_ring=ring, **kw)
        comp = _program(ring)
        runs = []
        for _ in range(3):
            r = rt.evaluate_computation(comp, {"x": x, "t": t})
            runs.append({n: r[f"output_{i}"] for i, n in enumerate(NAMES)})
        _RUNS[key] = runs
    return _RUNS[key]


def _check_outputs(outs, ring):
    f = FRAC[ring]
    x, t = _inputs(f)
    for name, (_fn, ref) in EXACT.items():
        want = ref(x, t)
        assert outs[name].shape == want.shape, name
        assert np.array_equal(outs[name], want), name
    for name, (_fn, ref, axis) in INTERPOLATED.items():
        n = x.shape[axis]
        pos = 0.5 * (n - 1) if name.startswith("median") else Q * (n - 1)
        s = np.sort(x, axis=axis)
        lo, hi = np.take(s, int(np.floor(pos)), axis=axis), np.take(s, int(np.ceil(pos)), axis=axis)
        # 2^-(f+1) of weight rounding times the gap, one TruncPr unit and one encoding unit
        tol = (np.abs(hi - lo) / 2 + 2) * 2.0 ** -f
        err = np.abs(outs[name] - ref(x, t))
        print(f"{name} ring{ring}: err {err.max():.3e} tol {tol.min():.3e}")
        assert outs[name].shape == err.shape and (err <= tol).all(), name


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("ring", (64, 128))
def test_order_statistics_match_numpy_and_replay(device, ring):
    runs = _evaluate_thrice(device, ring)
    for outs in runs:
        _check_outputs(outs, ring)
    for name in EXACT:  # exact results are equal in every evaluation (replays on a device)
        assert np.array_equal(runs[0][name], runs[1][name]), name
        assert np.array_equal(runs[0][name], runs[2][name]), name


def _exact_program(ring=128):
    return _program(ring, names=list(EXACT))


def test_stacked_and_per_party_threads_agree():
    comp = _exact_program()
    x, t = _inputs(40)
    stacked = LocalMooseRuntime(ROLES, device="cpu", seed=7).evaluate_computation(
        comp, {"x": x, "t": t})
    threads = LocalMooseRuntime(ROLES, device_map={r: "cpu" for r in ROLES},
                                seed=7).evaluate_computation(comp, {"x": x, "t": t})
    assert sorted(stacked) == sorted(threads)
    for i, name in enumerate(EXACT):
        assert np.array_equal(threads[f"output_{i}"], EXACT[name][1](x, t)), name
        assert np.array_equal(stacked[f"output_{i}"], threads[f"output_{i}"]), name


@pytest.mark.gpu
def test_per_party_threads_on_a_device():
    comp = _program(128, names=["sort", "sort_rows", "top_k"])
    x, t = _inputs(40)
    out = LocalMooseRuntime(ROLES, device_map={r: "cuda:0" for r in ROLES},
                            seed=7).evaluate_computation(comp, {"x": x, "t": t})
    for i, name in enumerate(["sort", "sort_rows", "top_k"]):
        assert np.array_equal(out[f"output_{i}"], EXACT[name][1](x, t)), name


def test_lowered_graph_takes_no_new_operator_and_agrees():
    names = ["sort", "sort_axis0_desc", "sort_rows", "top_k", "median_odd"]
    comp = _program(128, names=names)
    x, t = _inputs(40)
    low = passes.compile(to_native(comp), arg_specs={"x": x.shape, "t": t.shape})
    assert passes.is_lowered(low)
    passes.well_formed(low)
    kinds = {o.kind for o in low.operations}
    assert not kinds & {"Sort", "CswapDiff", "CswapApply", "CswapCross"}
    assert {"Reshape", "IndexAxis", "Sub", "Mul", "Add", "Concat"} <= kinds
    out = LocalMooseRuntime(ROLES, device="cpu", seed=7).evaluate_compiled(
        Computation.from_textual(low.to_textual()), {"x": x, "t": t})
    for i, name in enumerate(names):
        assert np.array_equal(out[f"output_{i}"], EXACT[name][1](x, t)), name


def test_serialised_forms_round_trip():
    native = to_native(_program(128, names=["sort_axis0_desc", "sort_rows"]))
    ops = [o for o in native.operations if o.kind == "Sort"]
    assert len(ops) == 2
    assert (ops[0].attrs["axis"], bool(ops[0].attrs["descending"]), ops[0].attrs["by"]) == \
        (0, True, -1)
    assert (ops[1].attrs["axis"], bool(ops[1].attrs["descending"]), ops[1].attrs["by"]) == \
        (0, False, 1)
    txt = native.to_textual()
    assert "Sort{" in txt and "by = 1" in txt
    assert Computation.from_textual(txt).to_textual() == txt
    assert Computation.from_msgpack(native.to_msgpack()).to_textual() == txt
    traced = tracer.trace(_program(128, names=["sort_rows"]))
    so = [o for o in traced.operations.values() if type(o).__name__ == "SortOperation"]
    assert so and so[0].by == 1 and so[0].axis == 0


@pytest.mark.parametrize("fixed", (False, True))
def test_a_host_placement_sorts_plaintext(fixed):
    @pm.computation
    def prog(x: pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64)),
             t: pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64))):
        with ALICE:
            if fixed:
                x, t = (pm.cast(v, dtype=DTYPES[128]) for v in (x, t))
            ys = (pm.sort(x, axis=0, descending=True), pm.sort_rows(t, by=1),
                  pm.top_k(x, 2, axis=1), pm.sort(x))
            return tuple(pm.cast(y, dtype=pm.float64) for y in ys) if fixed else ys

    x, t = _inputs(40)
    out = LocalMooseRuntime(ROLES, device="cpu").evaluate_computation(prog, {"x": x, "t": t})
    for i, name in enumerate(("sort_axis0_desc", "sort_rows")):
        assert np.array_equal(out[f"output_{i}"], EXACT[name][1](x, t)), name
    assert np.array_equal(out["output_2"], -np.sort(-x, axis=1)[:, :2])
    assert np.array_equal(out["output_3"], np.sort(x, axis=-1))


def test_trace_time_errors():
    with pytest.raises(ValueError, match="`median` needs the static length.*input_shape="):
        tracer.trace(_program(128, names=["median_odd"], shapes=False))
    with pytest.raises(ValueError, match="`quantile` needs the static length.*input_shape="):
        tracer.trace(_program(128, names=["q_lower"], shapes=False))
    tracer.trace(_program(128, names=["sort", "sort_rows"], shapes=False))  # no length needed

    def trace(fn):
        @pm.computation
        def prog(x: pm.Argument(placement=ALICE, vtype=pm.TensorType(DTYPES[128]), shape=XS)):
            with REP:
                y = fn(x)
            with CAROLE:
                return pm.identity(y)

        return tracer.trace(prog)

    trace(lambda v: pm.median(v, input_shape=XS))
    with pytest.raises(ValueError, match="`quantile`: interpolation must be one of"):
        trace(lambda v: pm.quantile(v, 0.5, interpolation="nearest"))
    with pytest.raises(ValueError, match="`quantile`: q must be"):
        trace(lambda v: pm.quantile(v, 1.5))
    with pytest.raises(ValueError, match="`top_k`: k = 9 exceeds"):
        trace(lambda v: pm.top_k(v, 9))
    with pytest.raises(ValueError, match="`sort_rows` expects a rank-2 tensor with more than 7"):
        trace(lambda v: pm.sort_rows(v, by=7))
    with pytest.raises(ValueError, match="`sort`: axis 2 out of range"):
        trace(lambda v: pm.sort(v, axis=2))


def test_a_dtype_without_room_for_the_difference_is_rejected_when_run():
    """fixed(40, 23) in Z_2^64: a difference takes 65 bits."""
    @pm.computation
    def prog(x: pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64))):
        with ALICE:
            xf = pm.cast(x, dtype=pm.fixed(40, 23))
        with REP:
            y = pm.sort(xf)
        with CAROLE:
            return pm.cast(y, dtype=pm.float64)

    rt = LocalMooseRuntime(ROLES, device="cpu", fixedpoint_ring=64)
    with pytest.raises(Exception, match=r"sort.*integral \+ fractional \+ 2"):
        rt.evaluate_computation(prog, {"x": np.zeros((2, 4))})
