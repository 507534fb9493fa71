"""rep.shuffle: one step against a Python-integer model, and the whole protocol on a seeded
stacked session -- consistent sharing, the input's rows as a multiset, re-randomised slots,
seeds, rounds and messages -- then with the parties as threads, as SPMD processes, and as a
lowered graph of PermFromKeys / PermGather."""
import numpy as np
import pytest
import torch

import moose_amd as pm
from moose_amd.compiler import passes
from moose_amd.ir.computation import Computation
from moose_amd.ir.computation import ReplicatedPlacement
from moose_amd.ops import ring as R
from moose_amd.protocols import fixedpoint as fxp
from moose_amd.protocols import replicated as rep
from moose_amd.runtime.local import LocalMooseRuntime
from moose_amd.runtime.local import to_native
from moose_amd.runtime.session import HV
from moose_amd.runtime.session import StackedSession

OWNERS = ("a", "b", "c")
PLC = ReplicatedPlacement(OWNERS)
DEVICES = ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)]
CASES = [((7,), 0), ((7,), -1), ((64, 3), 0), ((64, 3), 1), ((64, 3), -1), ((2, 16, 5), 0),
         ((2, 16, 5), 1), ((2, 16, 5), -1)]


def _values(shape, bits):
    """Distinct ring values with 0 and 2^bits - 1 among them."""
    n = int(np.prod(shape))
    top = (1 << bits) - 1
    v = [((k + 1) * 0x9E3779B97F4A7C15F39CC0605CEDC835) & top for k in range(n)]
    v[0], v[-1] = 0, top
    return np.array(v, dtype=object).reshape(shape)


def _share(sess, vals, bits, device):
    return rep.share(sess, PLC, HV("a", R.from_ints(vals, bits, device)))


def _reveal(sess, x):
    return R.to_ints(R.RT(rep.reveal(sess, x, "c").v.data.cpu(), x.bits))


def _rows(a, axis):
    """The slices of ``a`` along ``axis`` as a sorted list of tuples."""
    a = np.moveaxis(np.asarray(a, dtype=object), axis, 0)
    a = a.reshape(a.shape[0], -1)
    return sorted(tuple(int(v) for v in r) for r in a)


def _slots(x):
    """The three slots x_0, x_1, x_2 (s0 of every party) as integer arrays."""
    return [R.to_ints(R.RT(x.s0.v.data[j].cpu(), x.bits)) for j in range(3)]


def _step_model(xs, i, pi, r, s, mod):
    """Python-integer model of step i on the slots xs = (x_0, x_1, x_2): y_i = r, y_{i-1} =
    pi(x_{i-1} + x_i) - s, y_{i+1} = pi(x_{i+1}) + s - r; the slots sum to pi(x)."""
    y = [None] * 3
    y[i] = r % mod
    y[(i - 1) % 3] = ((xs[(i - 1) % 3] + xs[i])[pi] - s) % mod
    y[(i + 1) % 3] = (xs[(i + 1) % 3][pi] + s - r) % mod
    assert ((y[0] + y[1] + y[2]) % mod == ((xs[0] + xs[1] + xs[2]) % mod)[pi]).all()
    return y


# The stacked session expands a PRF key for whichever host asks, so the tests on it cannot tell
# a wrong holder of k_i from the right one.  The per-party sessions can -- there a party that
# does not hold the key draws from another slot and the rows come out wrong: the key-to-holder
# mapping of a step is guarded by test_parties_as_threads and test_spmd_processes_over_gloo.
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("i", [0, 1, 2])
def test_one_step_equals_the_integer_model(device, bits, i):
    """The slots a step leaves, against the model (whose slots sum to pi(x)) on the masks and
    the permutation a second session with the same seed derives from key k_i and the step's
    three nonces."""
    vals = _values((6, 3), bits)
    mod = 1 << bits
    sess = StackedSession(device, seed=21)
    x = _share(sess, vals, bits, device)
    before = {k: v for k, v in sess.stats.messages.items()}
    y = rep._shuffle_step(sess, x, i, 0, 6)
    sent = {k: v - before.get(k, 0) for k, v in sess.stats.messages.items()
            if v - before.get(k, 0)}
    c = OWNERS[(i + 1) % 3]  # both messages go to the outsider
    assert sent == {(OWNERS[(i - 1) % 3], c): 1, (OWNERS[i], c): 1}

    twin = StackedSession(device, seed=21)
    xs = _slots(_share(twin, vals, bits, device))
    h = OWNERS[i]
    n_perm, n_r, n_s = twin.nonce(PLC), twin.nonce(PLC), twin.nonce(PLC)
    pi = R.perm_from_keys(twin.h_prf(PLC, h, i, HV(h, (6,)), 64, n_perm).v).cpu().numpy()
    r = R.to_ints(R.RT(twin.h_prf(PLC, h, i, HV(h, (6, 3)), bits, n_r).v.data.cpu(), bits))
    s = R.to_ints(R.RT(twin.h_prf(PLC, h, i, HV(h, (6, 3)), bits, n_s).v.data.cpu(), bits))
    want = _step_model(xs, i, pi, r, s, mod)
    got = _slots(y)
    for j in range(3):
        assert (got[j] == want[j]).all(), j
    assert (_reveal(sess, y) == vals[pi]).all()


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("shape,axis", CASES)
def test_shuffle_keeps_the_rows_and_rerandomises_the_shares(device, bits, shape, axis):
    vals = _values(shape, bits)
    sess = StackedSession(device, seed=5)
    x = _share(sess, vals, bits, device)
    rounds, msgs, nbytes = (sess.stats.rounds, dict(sess.stats.messages),
                            dict(sess.stats.bytes))
    y = rep.shuffle(sess, x, axis)
    # three rounds, six messages of the tensor's size: every directed link once
    assert sess.stats.rounds - rounds == 3
    size = int(np.prod(shape)) * bits // 8
    links = {(p, q) for p in OWNERS for q in OWNERS if p != q}
    assert {k: v - msgs.get(k, 0) for k, v in sess.stats.messages.items()} == \
        {k: 1 for k in links}
    assert {k: v - nbytes.get(k, 0) for k, v in sess.stats.bytes.items()} == \
        {k: size for k in links}
    # consistent: s1 of party j is s0 of party j + 1, bitwise
    for j in range(3):
        assert torch.equal(y.s1.v.data[j], y.s0.v.data[(j + 1) % 3]), j
    out = _reveal(sess, y)
    assert out.shape == vals.shape
    assert _rows(out, axis) == _rows(vals, axis)  # whole rows, bit for bit, in some order
    n = shape[axis]
    if n == 64:
        assert not (out == vals).all()
    ins = [_rows(s, axis) for s in _slots(x)]  # the shares are re-randomised, not only moved
    for k, s in enumerate(_slots(y)):
        assert all(_rows(s, axis) != t for t in ins), k


@pytest.mark.parametrize("device", DEVICES)
def test_a_row_id_column_travels_with_its_row(device):
    ids = np.arange(64).astype(object)
    table = np.stack([ids, ids * 7 + 1, (1 << 64) - 1 - ids], axis=1).astype(object)
    sess = StackedSession(device, seed=9)
    out = _reveal(sess, rep.shuffle(sess, _share(sess, table, 64, device), 0))
    order = [int(v) for v in out[:, 0]]
    assert sorted(order) == list(range(64)) and order != list(range(64))
    assert (out == table[order]).all()


def test_seeds_fix_the_order():
    vals = _values((64, 3), 128)

    def run(seed):
        sess = StackedSession("cpu", seed=seed)
        return _reveal(sess, rep.shuffle(sess, _share(sess, vals, 128, "cpu"), 0))

    a, b, c = run(1), run(1), run(2)
    assert (a == b).all()
    assert not (a == c).all() and _rows(a, 0) == _rows(c, 0)


def test_edges_and_errors():
    sess = StackedSession("cpu", seed=3)
    one = _share(sess, _values((1, 4), 64), 64, "cpu")
    assert rep.shuffle(sess, one, 0) is one  # n <= 1: unchanged
    x = _share(sess, _values((4, 3), 64), 64, "cpu")
    with pytest.raises(ValueError, match="axis 2 out of range"):
        rep.shuffle(sess, x, 2)
    with pytest.raises(ValueError, match="axis -3 out of range"):
        rep.shuffle(sess, x, -3)
    bit = rep.share(sess, PLC, HV("a", R.from_ints(np.array([0, 1, 1, 0], dtype=object), 1)),
                    kind="bool")
    with pytest.raises(ValueError, match="bit sharing is not supported"):
        rep.shuffle(sess, bit, 0)
    f = fxp.shuffle(sess, fxp.RepFixed(x, 23, 14), -1)
    assert (f.frac, f.integ, f.bits) == (23, 14, 64)
    assert _rows(_reveal(sess, f.t), 1) == _rows(_values((4, 3), 64), 1)


# ---------------------------------------------------------------------------
# the other sessions, through the eDSL
# ---------------------------------------------------------------------------
ROLES = ["alice", "bob", "carole"]
ALICE, BOB, CAROLE = (pm.host_placement(n) for n in ROLES)
REP = pm.replicated_placement("rep", players=[ALICE, BOB, CAROLE])
SHAPE = (16, 3)


def _program(ring=128):
    dt = {64: pm.fixed(14, 23), 128: pm.fixed(24, 40)}[ring]

    @pm.computation
    def prog(x: pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64), shape=SHAPE)):
        with ALICE:
            xf = pm.cast(x, dtype=dt)
        with REP:
            y = pm.shuffle(xf)
            z = pm.shuffle(xf, axis=-1)
        with CAROLE:
            return pm.cast(y, dtype=pm.float64), pm.cast(z, dtype=pm.float64)

    return prog


def _table():
    ids = np.arange(SHAPE[0], dtype=np.float64)
    return np.stack([ids, ids * 0.5 - 3, -ids - 0.25], axis=1)


def _check_table(out):
    x = _table()
    y, z = out["output_0"], out["output_1"]
    order = [int(v) for v in y[:, 0]]
    assert sorted(order) == list(range(SHAPE[0]))
    assert np.array_equal(y, x[order])  # rows intact
    cols = [list(x[0]).index(v) for v in z[0]]
    assert sorted(cols) == [0, 1, 2] and np.array_equal(z, x[:, cols])


def test_parties_as_threads():
    rt = LocalMooseRuntime(ROLES, device_map={r: "cpu" for r in ROLES}, seed=7)
    _check_table(rt.evaluate_computation(_program(), {"x": _table()}))


@pytest.mark.gpu
def test_parties_as_threads_on_a_device():
    rt = LocalMooseRuntime(ROLES, device_map={r: "cuda:0" for r in ROLES}, seed=7)
    _check_table(rt.evaluate_computation(_program(), {"x": _table()}))


def test_spmd_processes_over_gloo():
    from moose_amd.runtime.distributed import DistributedMooseRuntime

    with DistributedMooseRuntime(ROLES, backend="gloo", seed=3, timeout=60) as rt:
        _check_table(rt.evaluate_computation(_program(), {"x": _table()}))


@pytest.mark.parametrize("ring", [64, 128])
def test_lowered_graph_runs_on_the_two_host_operators(ring):
    x = _table()
    low = passes.compile(to_native(_program(ring), ring), arg_specs={"x": x.shape},
                         fixedpoint_ring=ring)
    assert passes.is_lowered(low)
    passes.well_formed(low)
    kinds = [o.kind for o in low.operations]
    assert "Shuffle" not in kinds
    # two shuffles x three steps x two holders
    assert kinds.count("PermFromKeys") == 12 and kinds.count("PermGather") == 12
    forms = sorted(o.attrs["form"] for o in low.operations if o.kind == "PermGather")
    assert forms == ["bm"] * 6 + ["pm"] * 6
    txt = low.to_textual()
    assert "PermGather{" in txt and "PermFromKeys" in txt
    again = Computation.from_textual(txt)
    assert again.to_textual() == txt
    assert Computation.from_bincode(low.to_bincode()).to_textual() == txt
    out = LocalMooseRuntime(ROLES, device="cpu", fixedpoint_ring=ring).evaluate_compiled(
        again, {"x": x})
    _check_table(out)


def test_serialised_forms_round_trip():
    native = to_native(_program())
    ops = [o for o in native.operations if o.kind == "Shuffle"]
    assert [o.attrs["axis"] for o in ops] == [0, 1]  # the negative axis resolved at trace time
    txt = native.to_textual()
    assert "Shuffle{" in txt
    assert Computation.from_textual(txt).to_textual() == txt
    assert Computation.from_msgpack(native.to_msgpack()).to_textual() == txt
    assert Computation.from_bincode(native.to_bincode()).to_textual() == txt
