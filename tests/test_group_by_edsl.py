"""pm.group_by_sum, pm.group_by_count and pm.cumsum through the eDSL: a replicated placement
against the same operator on a host placement (the plaintext specification) and against numpy,
exactly -- the inputs are multiples of 2^-8 with |x| <= 16, so every sum is exact in float64 and
nothing in the protocol truncates; evaluated three times (replayed on a device without the final
shuffle, eager with it), the trace-time errors, and the serialised forms."""
import warnings

import numpy as np
import pytest

import moose_amd as pm
from moose_amd.ir.computation import Computation
from moose_amd.runtime import graphs
from moose_amd.runtime.local import LocalMooseRuntime
from moose_amd.runtime.local import to_native

ROLES = ["alice", "bob", "carole"]
ALICE, BOB, CAROLE = (pm.host_placement(n) for n in ROLES)
REP = pm.replicated_placement("rep", players=[ALICE, BOB, CAROLE])
DEVICES = ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)]
# (dtype, ring): fixed(14, 23) over both rings and fixed(24, 40) over Z_2^128
CONFIGS = {"f14_23_r64": (pm.fixed(14, 23), 64), "f14_23_r128": (pm.fixed(14, 23), 128),
           "f24_40_r128": (pm.fixed(24, 40), 128)}


def _grid(rng, shape):
    return rng.integers(-16 * 256, 16 * 256 + 1, size=shape) / 256.0


def _tables():
    """name -> (table, by, count)."""
    rng = np.random.default_rng(12)
    out = {"n1": (_grid(rng, (1, 3)), 0, False)}
    t = _grid(rng, (6, 3))
    t[:, 1] = 1.5
    out["all_equal"] = (t, 1, False)
    t = _grid(rng, (5, 2))
    t[:, 0] = rng.permutation(5) * 0.75 - 1.0
    out["all_distinct"] = (t, 0, False)
    t = _grid(rng, (8, 3))
    t[:, 0] = rng.choice([-3.5, -0.25, -16.0], size=8)
    out["negative_keys"] = (t, 0, False)
    t = _grid(rng, (37, 3))  # five groups of uneven size; 37 rows are padded to 64 by the sort
    t[:, 0] = np.repeat([7.0, -2.5, 0.0, 0.00390625, 15.5], [1, 20, 3, 11, 2])[rng.permutation(37)]
    out["n37"] = (t, 0, False)
    t = _grid(rng, (9, 2))
    t[:, 0] = rng.choice([1.0, 2.0, -1.0], size=9)
    out["count"] = (t, 0, True)
    t = _grid(rng, (7, 4))
    t[:, 3] = rng.choice([0.5, -0.5], size=7)
    out["by_last"] = (t, 3, True)
    return out


TABLES = _tables()


def _reference(t, by, count):
    """numpy: the rows sorted by the key; the last row of each group holds (key, sums of the
    other columns, the group's size if asked, 1.0), every other row zero."""
    n, c = t.shape
    s = t[np.argsort(t[:, by], kind="stable")]
    out = np.zeros((n, c + int(count) + 1))
    others = [i for i in range(c) if i != by]
    start = 0
    for i in range(n):
        if i == n - 1 or s[i + 1, by] != s[i, by]:
            row = [s[i, by]] + [s[start:i + 1, j].sum() for j in others]
            out[i] = row + ([float(i + 1 - start)] if count else []) + [1.0]
            start = i + 1
    return out


def _group_program(dt, name, shuffle=False, where="rep"):
    """group_by_sum of one table on the replicated placement, or on alice's in the clear."""
    t, by, count = TABLES[name]

    @pm.computation
    def prog(a: pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64), shape=t.shape)):
        with ALICE:
            f = pm.cast(a, dtype=dt)
        with (REP if where == "rep" else ALICE):
            r = pm.group_by_sum(f, by=by, count=count, shuffle=shuffle)
        with CAROLE:
            return pm.cast(r, dtype=pm.float64)

    return prog


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_group_by_sum_equals_the_host_and_numpy(device, config):
    dt, ring = CONFIGS[config]
    rt = LocalMooseRuntime(ROLES, device=device, fixedpoint_ring=ring)
    for name, (t, by, count) in TABLES.items():
        want = _reference(t, by, count)
        plain = _group_program(dt, name, where="host")
        assert not graphs.capturable(to_native(plain))  # a host's sort is not captured
        host = rt.evaluate_computation(plain, {"a": t})
        assert host["output_0"].shape == want.shape, name
        assert np.array_equal(host["output_0"], want), ("host", name)
        comp = _group_program(dt, name)
        assert graphs.capturable(to_native(comp))  # without the shuffle it is replayable
        for _ in range(3):  # the second and third evaluation (replays on a device) agree
            with warnings.catch_warnings():  # a capture that fails warns and runs eagerly
                warnings.filterwarnings("error", message="hipGraph capture failed")
                secure = rt.evaluate_computation(comp, {"a": t})["output_0"]
            assert secure.shape == want.shape, name
            assert np.array_equal(secure, want), ("replicated", name)


@pytest.mark.parametrize("device", DEVICES)
def test_a_final_shuffle_permutes_the_rows_and_stays_eager(device):
    dt, ring = CONFIGS["f24_40_r128"]
    rt = LocalMooseRuntime(ROLES, device=device, fixedpoint_ring=ring)
    rows = lambda a: sorted(tuple(r) for r in a.tolist())  # noqa: E731
    for name in ("n37", "count"):
        comp = _group_program(dt, name, shuffle=True)
        assert not graphs.capturable(to_native(comp))
        want = _reference(*TABLES[name])
        for _ in range(2):
            out = rt.evaluate_computation(comp, {"a": TABLES[name][0]})
            assert rows(out["output_0"]) == rows(want), name
        host = _group_program(dt, name, shuffle=True, where="host")  # a host does not shuffle
        assert np.array_equal(rt.evaluate_computation(host, {"a": TABLES[name][0]})["output_0"],
                              want)


ATTRS = [(ex, rev) for ex in (False, True) for rev in (False, True)]
XS = (5, 7)


def _np_cumsum(x, axis, exclusive, reverse):
    a = np.flip(x, axis) if reverse else x
    c = np.cumsum(a, axis=axis)
    if exclusive:
        c = c - a
    return np.flip(c, axis) if reverse else c


def _scan_program(dt):
    @pm.computation
    def prog(x: pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64), shape=XS),
             t: pm.Argument(placement=BOB, vtype=pm.TensorType(pm.float64), shape=(9, 3))):
        outs = []
        with ALICE:
            xf = pm.cast(x, dtype=dt)
            host = [pm.cumsum(xf, axis=0, exclusive=ex, reverse=rev) for ex, rev in ATTRS]
            flt = [pm.cumsum(x, axis=1, exclusive=ex, reverse=rev) for ex, rev in ATTRS]
        with BOB:
            tf = pm.cast(t, dtype=dt)
        with REP:
            for axis in (0, -1):
                outs += [pm.cumsum(xf, axis=axis, exclusive=ex, reverse=rev) for ex, rev in ATTRS]
            cnt = pm.group_by_count(tf, by=1, shuffle=False)
        with CAROLE:
            return tuple(pm.cast(y, dtype=pm.float64) for y in outs + host + [cnt]) + tuple(flt)

    return prog


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_cumsum_and_group_by_count_match_numpy(device, config):
    dt, ring = CONFIGS[config]
    rng = np.random.default_rng(5)
    x, t = _grid(rng, XS), _grid(rng, (9, 3))
    t[:, 1] = rng.choice([3.0, -4.25], size=9)
    rt = LocalMooseRuntime(ROLES, device=device, fixedpoint_ring=ring)
    comp = _scan_program(dt)
    for _ in range(3):
        out = rt.evaluate_computation(comp, {"x": x, "t": t})
        got = [out[f"output_{i}"] for i in range(len(out))]
        want = [_np_cumsum(x, axis, ex, rev) for axis in (0, 1) for ex, rev in ATTRS]
        want += [_np_cumsum(x, 0, ex, rev) for ex, rev in ATTRS]
        want += [_reference(t[:, 1:2], 0, True)]
        want += [_np_cumsum(x, 1, ex, rev) for ex, rev in ATTRS]
        assert len(got) == len(want) == 17
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and np.array_equal(g, w), k


def test_trace_time_errors():
    f = pm.fixed(14, 23)

    def trace(body, **kw):
        @pm.computation
        def prog(x: pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64), **kw)):
            with ALICE:
                xf = pm.cast(x, dtype=f)
            with REP:
                y = body(xf)
            with CAROLE:
                return pm.cast(y, dtype=pm.float64)

        return to_native(prog)

    with pytest.raises(ValueError, match="rank-2"):
        trace(lambda x: pm.group_by_sum(x), shape=(4,))
    with pytest.raises(ValueError, match="rank-2"):
        trace(lambda x: pm.group_by_count(x), shape=(4, 2, 2))
    with pytest.raises(ValueError, match="more than 3 columns"):
        trace(lambda x: pm.group_by_sum(x, by=3), shape=(4, 3))
    with pytest.raises(ValueError, match="column index"):
        trace(lambda x: pm.group_by_sum(x, by=-1), shape=(4, 3))
    with pytest.raises(ValueError, match="`group_by_sum` needs the static"):
        trace(lambda x: pm.group_by_sum(x))
    with pytest.raises(ValueError, match="`group_by_count` needs the static"):
        trace(lambda x: pm.group_by_count(x))
    with pytest.raises(ValueError, match="bit tensors"):
        trace(lambda x: pm.group_by_sum(pm.less(x, x)), shape=(4, 3))
    with pytest.raises(ValueError, match="bit tensors"):
        trace(lambda x: pm.cumsum(pm.less(x, x)), shape=(4, 3))
    with pytest.raises(ValueError, match="out of range"):
        trace(lambda x: pm.cumsum(x, axis=2), shape=(4, 3))
    # input_shape= stands in for a missing static shape
    comp = trace(lambda x: pm.group_by_sum(x, by=1, count=True, input_shape=(4, 3)))
    assert [o.kind for o in comp.operations].count("GroupBySum") == 1


def test_serialised_forms_round_trip():
    native = to_native(_scan_program(pm.fixed(14, 23)))
    kinds = [o.kind for o in native.operations]
    assert kinds.count("CumSum") == 16 and kinds.count("GroupBySum") == 1
    op = next(o for o in native.operations if o.kind == "GroupBySum")
    assert (op.attrs["by"], op.attrs["count"], op.attrs["shuffle"]) == (0, True, False)
    txt = native.to_textual()
    assert "CumSum{" in txt and "GroupBySum{" in txt
    assert Computation.from_textual(txt).to_textual() == txt
    assert Computation.from_msgpack(native.to_msgpack()).to_textual() == txt
