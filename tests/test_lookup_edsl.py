"""pm.one_hot, pm.lookup and pm.bincount through the eDSL: a host placement (the plaintext
specification) and the replicated placement against numpy, exactly -- every value is a
multiple of 2^-8 with |x| <= 16, so it is exact in both encodings and nothing in the protocol
truncates; an argmax as the index, bincount against group_by_sum, replay against the first
evaluation on a device, the serialised forms and the errors."""
import warnings

import numpy as np
import pytest

import moose_amd as pm
from moose_amd.computation import utils as comp_utils
from moose_amd.edsl import tracer
from moose_amd.ir.computation import Computation
from moose_amd.runtime import graphs
from moose_amd.runtime.local import LocalMooseRuntime
from moose_amd.runtime.local import to_native

ROLES = ["alice", "bob", "carole"]
ALICE, BOB, CAROLE = (pm.host_placement(n) for n in ROLES)
REP = pm.replicated_placement("rep", players=[ALICE, BOB, CAROLE])
DEVICES = ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)]
CONFIGS = {"f14_23_r64": (pm.fixed(14, 23), 64), "f24_40_r128": (pm.fixed(24, 40), 128)}

RNG = np.random.default_rng(41)
grid = lambda shape: RNG.integers(-16 * 256, 16 * 256 + 1, size=shape) / 256.0  # noqa: E731
T2 = grid((11, 3))                      # 13 indices into [11, 3]
I2 = np.concatenate([np.arange(11), [10, 0]]).astype(np.float64)[RNG.permutation(13)]
T1 = grid((16,))                        # 13 indices into [16]
I1 = np.concatenate([[15, 0], RNG.integers(0, 16, size=11)]).astype(np.float64)
W = grid((40, 2))                       # 40 rows into 5 bins
K = np.concatenate([np.arange(5), RNG.integers(0, 5, size=35)]).astype(np.float64)
CONST = grid((11, 3))
ARGS = {"t2": T2, "i2": I2, "t1": T1, "i1": I1, "w": W, "k": K}


def _arg(a, who=ALICE):
    return pm.Argument(placement=who, vtype=pm.TensorType(pm.float64), shape=a.shape)


def _program(dt, where):
    plc = REP if where == "rep" else ALICE

    @pm.computation
    def prog(t2: _arg(T2), i2: _arg(I2, BOB), t1: _arg(T1), i1: _arg(I1, BOB), w: _arg(W),
             k: _arg(K, BOB)):
        with ALICE:
            t2f, t1f, wf = (pm.cast(v, dtype=dt) for v in (t2, t1, w))
        with BOB:
            i2f, i1f, kf = (pm.cast(v, dtype=dt) for v in (i2, i1, k))
        with plc:
            outs = [pm.one_hot(i2f, 11), pm.lookup(t2f, i2f),
                    pm.lookup(pm.constant(CONST, dtype=dt), i2f), pm.lookup(t1f, i1f),
                    pm.bincount(kf, 5), pm.bincount(kf, 5, weights=wf),
                    pm.one_hot(i1f, 13)]  # the indices 13..15 select nothing
        with CAROLE:
            return tuple(pm.cast(o, dtype=pm.float64) for o in outs)

    return prog


def _want():
    i2, i1, k = I2.astype(int), I1.astype(int), K.astype(int)
    oh13 = np.eye(16)[i1][:, :13]
    return [np.eye(11)[i2], T2[i2], CONST[i2], T1[i1], np.bincount(k, minlength=5).astype(float),
            np.eye(5)[k].T @ W, oh13]


def _check(out):
    want = _want()
    assert len(out) == len(want)
    for j, w in enumerate(want):
        got = out[f"output_{j}"]
        assert got.shape == w.shape, (j, got.shape, w.shape)
        assert np.array_equal(got, w), j


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_equals_numpy_on_a_host_and_replicated(device, config):
    dt, ring = CONFIGS[config]
    rt = LocalMooseRuntime(ROLES, device=device, fixedpoint_ring=ring)
    _check(rt.evaluate_computation(_program(dt, "host"), ARGS))
    comp = _program(dt, "rep")
    assert graphs.capturable(to_native(comp))  # all three are static
    first = None
    for _ in range(2):  # the second evaluation is a replay on a device
        with warnings.catch_warnings():
            warnings.filterwarnings("error", message="hipGraph capture failed")
            out = rt.evaluate_computation(comp, ARGS)
        _check(out)
        first = first or out
        assert all(np.array_equal(out[k], first[k]) for k in out)


def test_parties_as_threads():
    dt, ring = CONFIGS["f24_40_r128"]
    rt = LocalMooseRuntime(ROLES, device_map={r: "cpu" for r in ROLES}, fixedpoint_ring=ring)
    _check(rt.evaluate_computation(_program(dt, "rep"), ARGS))


@pytest.mark.parametrize("device", DEVICES)
def test_an_argmax_is_an_index(device):
    dt = pm.fixed(24, 40)
    scores = grid((9, 6))
    scores[np.arange(9), np.arange(9) % 6] = 16.5  # a unique maximum per row
    table = grid((6, 4))

    @pm.computation
    def prog(s: _arg(scores), t: _arg(table, BOB)):
        with ALICE:
            sf = pm.cast(s, dtype=dt)
        with BOB:
            tf = pm.cast(t, dtype=dt)
        with REP:
            i = pm.argmax(sf, axis=1, upmost_index=6)
            outs = (pm.lookup(tf, i), pm.one_hot(i, 6, dtype=dt), pm.bincount(i, 6))
        with CAROLE:
            return tuple(pm.cast(o, dtype=pm.float64) for o in outs)

    out = LocalMooseRuntime(ROLES, device=device, fixedpoint_ring=128).evaluate_computation(
        prog, {"s": scores, "t": table})
    i = np.argmax(scores, axis=1)
    assert np.array_equal(out["output_0"], table[i])
    assert np.array_equal(out["output_1"], np.eye(6)[i])
    assert np.array_equal(out["output_2"], np.bincount(i, minlength=6).astype(float))


def test_bincount_agrees_with_group_by_sum():
    dt = pm.fixed(24, 40)
    table = np.concatenate([K[:, None], W], axis=1)  # keys 0..4

    @pm.computation
    def prog(t: _arg(table)):
        with ALICE:
            tf = pm.cast(t, dtype=dt)
        with REP:
            key = pm.squeeze(pm.strided_slice(tf, [slice(0, 40), slice(0, 1)]), axis=1)
            vals = pm.strided_slice(tf, [slice(0, 40), slice(1, 3)])
            outs = (pm.bincount(key, 5, weights=vals), pm.group_by_sum(tf, by=0, shuffle=False))
        with CAROLE:
            return tuple(pm.cast(o, dtype=pm.float64) for o in outs)

    out = LocalMooseRuntime(ROLES, device="cpu", fixedpoint_ring=128).evaluate_computation(
        prog, {"t": table})
    bins, groups = out["output_0"], out["output_1"]
    valid = groups[groups[:, -1] == 1.0]
    assert np.array_equal(valid[:, 0], np.arange(5.0))  # every key occurs
    assert np.array_equal(valid[:, 1:3], bins)


def test_serialised_forms_round_trip():
    prog = _program(pm.fixed(14, 23), "rep")
    native = to_native(prog)
    kinds = [o.kind for o in native.operations]
    assert (kinds.count("OneHot"), kinds.count("Lookup"), kinds.count("BinCount")) == (2, 3, 2)
    assert sorted(o.attrs["depth"] for o in native.operations if o.kind == "OneHot") == [11, 13]
    assert [o.attrs["length"] for o in native.operations if o.kind == "BinCount"] == [5, 5]
    assert sorted(len(o.inputs) for o in native.operations if o.kind == "BinCount") == [1, 2]
    txt = native.to_textual()
    assert "OneHot{" in txt and "Lookup" in txt and "BinCount{" in txt
    assert Computation.from_textual(txt).to_textual() == txt
    traced = tracer.trace(prog)
    again = comp_utils.deserialize_computation(comp_utils.serialize_computation(traced))
    ops = {type(o).__name__: o for o in again.operations.values()}
    assert ops["OneHotOperation"].depth in (11, 13) and ops["BinCountOperation"].length == 5
    assert "LookupOperation" in ops
    assert to_native(again).to_textual() == txt


def test_errors_carry_the_operator():
    f = pm.fixed(14, 23)

    def trace(body, shape=(4,), tshape=(4, 3)):
        @pm.computation
        def prog(x: pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64), shape=shape),
                 t: pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64), shape=tshape)):
            with ALICE:
                xf, tf = pm.cast(x, dtype=f), pm.cast(t, dtype=f)
            with REP:
                y = body(xf, tf)
            with CAROLE:
                return pm.cast(y, dtype=pm.float64)

        return to_native(prog)

    for bad in (0, -3, True, 2.5):
        with pytest.raises(ValueError, match=r"`one_hot`: `depth`.*" + repr(bad)):
            trace(lambda x, t: pm.one_hot(x, bad))
        with pytest.raises(ValueError, match=r"`bincount`: `length`.*" + repr(bad)):
            trace(lambda x, t: pm.bincount(x, bad))
    for name, body in (("one_hot", lambda x, t: pm.one_hot(pm.less(x, x), 4)),
                       ("lookup", lambda x, t: pm.lookup(t, pm.less(x, x))),
                       ("lookup", lambda x, t: pm.lookup(pm.less(t, t), x)),
                       ("bincount", lambda x, t: pm.bincount(pm.less(x, x), 4)),
                       ("bincount", lambda x, t: pm.bincount(x, 4, weights=pm.less(t, t)))):
        with pytest.raises(ValueError, match=f"`{name}`.*bit tensors"):
            trace(body)
    with pytest.raises(ValueError, match="`lookup` needs a table.*leading size"):
        trace(lambda x, t: pm.lookup(t, x), tshape=None)
    comp = trace(lambda x, t: pm.lookup(t, x, input_shape=(4, 3)), tshape=None)
    assert [o.kind for o in comp.operations].count("Lookup") == 1


def test_a_table_and_index_on_different_placements_are_refused():
    """The interpreter moves both operands to the operator's placement, so the check is
    reached at the fixed-point level: a secret table and an index of two replicated placements."""
    from moose_amd.ir.computation import ReplicatedPlacement
    from moose_amd.ops import ring as R
    from moose_amd.protocols import fixedpoint as fxp
    from moose_amd.protocols import replicated as rep
    from moose_amd.runtime.session import HV
    from moose_amd.runtime.session import StackedSession

    sess = StackedSession("cpu", seed=31)
    here, there = ReplicatedPlacement(("a", "b", "c")), ReplicatedPlacement(("b", "c", "d"))
    ints = lambda v: R.from_ints(np.array(v, dtype=object), 64, "cpu")  # noqa: E731
    table = fxp.RepFixed(rep.share(sess, here, HV("a", ints([[1, 2], [3, 4], [5, 6]]))), 0, 14)
    idx = rep.share(sess, there, HV("b", ints([0, 2])))
    with pytest.raises(ValueError, match=r"lookup: the table is on .*\('a', 'b', 'c'\).* and "
                                         r"the index on .*\('b', 'c', 'd'\)"):
        fxp.lookup(sess, table, idx)
    same = rep.share(sess, here, HV("a", ints([0, 2])))
    got = rep.reveal(sess, fxp.lookup(sess, table, same), "c")
    assert (R.to_ints(R.RT(got.v.data, 64)) == np.array([[1, 2], [5, 6]], dtype=object)).all()
