"""rep.demux on a seeded stacked session against the integer one-hot, exactly: every index
value of every width on both rings, rows whose index is past the last output, the invariant
of every group after every level, and the rounds and launches a demultiplexer costs."""
import numpy as np
import pytest

from moose_amd.ir.computation import ReplicatedPlacement
from moose_amd.ops import ring as R
from moose_amd.protocols import replicated as rep
from moose_amd.runtime.session import HV
from moose_amd.runtime.session import StackedSession

PLC = ReplicatedPlacement(("a", "b", "c"))
DEVICES = ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)]
SIZES = (1, 2, 3, 4, 5, 8, 11, 16, 33)
ROWS = 7


def _share(sess, vals, bits, device):
    enc = np.vectorize(lambda v: int(v) % (1 << bits), otypes=[object])(vals)
    return rep.share(sess, PLC, HV("a", R.from_ints(enc, bits, device)))


def _reveal(sess, x):
    return R.to_ints(R.RT(rep.reveal(sess, x, "c").v.data.cpu(), x.bits))


def _indices(n, rows=ROWS):
    """``rows`` indices over [0, 2^w) with every value present at least once where rows allow,
    the largest and 0 always; more rows than ROWS where 2^w is larger."""
    w = rep.demux_width(n)
    rows = max(rows, 1 << w)
    idx = np.arange(rows) % (1 << w)
    return w, idx[::-1].copy()


def _planes(idx, w):
    return np.array([[(int(i) >> t) & 1 for i in idx] for t in range(w)], dtype=object)


def _one_hot(idx, n):
    out = np.zeros((len(idx), n), dtype=object)
    for r, i in enumerate(idx):
        if i < n:
            out[r, i] = 1
    return out


class _Launches:
    """A session's p_outer_cross, counted per call."""

    def __init__(self, sess):
        self.geoms, self._f = [], sess.p_outer_cross
        sess.p_outer_cross = self

    def __call__(self, plc, x0, x1, geom, *y):
        self.geoms.append(geom)
        return self._f(plc, x0, x1, geom, *y)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bits", [64, 128])
def test_demux_equals_the_integer_one_hot(device, bits):
    sess = StackedSession(device, seed=21)
    for n in SIZES:
        w, idx = _indices(n)
        assert set(idx) == set(range(1 << w))  # every index value, those past n included
        seen = []
        got = rep.demux(sess, _share(sess, _planes(idx, w), bits, device), n,
                        on_level=lambda k, gs: seen.append((k, [_reveal(sess, g) for g in gs])))
        out = _reveal(sess, got)
        assert out.shape == (len(idx), n)
        if n == 1:  # nothing to select: public ones, whatever the bit holds
            assert (out == 1).all() and not seen
            continue
        assert (out == _one_hot(idx, n)).all(), (bits, n)
        assert (out[idx >= n] == 0).all()
        # after every level each group of each row is the one-hot of its own bits: group q
        # covers the bits [lo, lo + log2 size) in order
        levels = (w - 1).bit_length()
        assert [k for k, _ in seen] == list(range(levels + 1))
        for k, groups in seen:
            lo = 0
            for part in groups:
                for q in range(part.shape[0]):
                    size = part.shape[2]
                    nb = (size - 1).bit_length() if k < levels else w
                    sub = (idx >> lo) & ((1 << nb) - 1)
                    assert (part[q] == _one_hot(sub, size)).all(), (n, k, lo)
                    lo += nb
            assert lo == w


@pytest.mark.parametrize("n", SIZES + (100, 1000))
def test_a_demux_costs_one_round_per_level(n):
    sess = StackedSession("cpu", seed=22)
    w, idx = _indices(n, rows=3)
    planes = _share(sess, _planes(idx, w), 64, "cpu")
    spy = _Launches(sess)
    levels = []
    rounds = sess.stats.rounds
    rep.demux(sess, planes, n, on_level=lambda k, gs: levels.append(len(spy.geoms)))
    want = (w - 1).bit_length() if n > 1 else 0  # ceil(log2 w)
    # the session counts one reshare per launch; the two of one level do not depend on each
    # other, so a level is one round of communication
    assert sess.stats.rounds - rounds == len(spy.geoms)
    if n > 1:
        per_level = np.diff(levels)
        assert len(per_level) == want and all(1 <= c <= 2 for c in per_level), (n, per_level)
        if want:
            assert spy.geoms[-1].n_out == n
            assert all(g.n_out == g.A * g.B for g in spy.geoms[:-1])
    else:
        assert not spy.geoms


def test_errors():
    sess = StackedSession("cpu", seed=23)
    planes = _share(sess, _planes(np.arange(4), 2), 64, "cpu")
    for bad in (0, -1, True, 2.0):
        with pytest.raises(ValueError, match="positive integer"):
            rep.demux(sess, planes, bad)
    with pytest.raises(ValueError, match=r"\[3, rows\]"):
        rep.demux(sess, planes, 5)
    bit = rep.RepTensor(PLC, 1, "bool", planes.s0, planes.s1)
    with pytest.raises(ValueError, match="arithmetic"):
        rep.demux(sess, bit, 4)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bits", [64, 128])
def test_bits_above_the_width_are_ignored(device, bits):
    """An index with bits set above w gives the row of idx mod 2^w: as a uint64 ring tensor
    (bit t) and as a fixed-point tensor (bit frac + t, fractional bits ignored too)."""
    from moose_amd.protocols import fixedpoint as fxp

    sess = StackedSession(device, seed=24)
    n, frac = 11, 23
    w = rep.demux_width(n)
    low = np.arange(1 << w)
    high = np.array([0, 1 << w, 5 << w, (1 << 20) + (1 << w)] * 4, dtype=object)
    idx = low.astype(object) + high
    want = _one_hot(low, n)
    got = fxp.one_hot(sess, _share(sess, idx, 64, device), n, 0, 0, bits)
    assert (_reveal(sess, got.t) == want).all()
    fixed = idx * (1 << frac) + np.arange(len(idx)) * 12345 % (1 << frac)
    x = fxp.RepFixed(_share(sess, fixed, bits, device), frac, 14)
    got = fxp.one_hot(sess, x, n, frac, 14, bits)
    assert (_reveal(sess, got.t) == want * (1 << frac)).all()


# ---------------------------------------------------------------------------
# the other sessions, through the eDSL
# ---------------------------------------------------------------------------
import moose_amd as pm  # noqa: E402
from moose_amd.compiler import passes  # noqa: E402
from moose_amd.ir.computation import Computation  # noqa: E402
from moose_amd.runtime.local import LocalMooseRuntime  # noqa: E402
from moose_amd.runtime.local import to_native  # noqa: E402

ROLES = ["alice", "bob", "carole"]
ALICE, BOB, CAROLE = (pm.host_placement(r) for r in ROLES)
REP = pm.replicated_placement("rep", players=[ALICE, BOB, CAROLE])
INDEX = np.array([0, 32, 7, 33, 63, 5, 40, 32, 1], dtype=np.float64)  # n = 33: w = 6
TABLE = np.arange(33 * 2, dtype=np.float64).reshape(33, 2) / 4 - 3


def _program(ring=128):
    dt = {64: pm.fixed(14, 23), 128: pm.fixed(24, 40)}[ring]

    @pm.computation
    def prog(i: pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64), shape=INDEX.shape),
             t: pm.Argument(placement=BOB, vtype=pm.TensorType(pm.float64), shape=TABLE.shape)):
        with ALICE:
            x = pm.cast(i, dtype=dt)
        with BOB:
            tf = pm.cast(t, dtype=dt)
        with REP:
            outs = (pm.one_hot(x, 33), pm.one_hot(x, 5), pm.lookup(tf, x), pm.bincount(x, 33))
        with CAROLE:
            return tuple(pm.cast(o, dtype=pm.float64) for o in outs)

    return prog


def _check_program(out):
    idx = INDEX.astype(int)
    oh = _one_hot(idx, 33).astype(np.float64)
    assert np.array_equal(out["output_0"], oh)
    assert np.array_equal(out["output_1"], _one_hot(idx % 8, 5).astype(np.float64))
    assert np.array_equal(out["output_2"], oh @ TABLE)
    assert np.array_equal(out["output_3"], oh.sum(0))


def test_stacked_session():
    _check_program(LocalMooseRuntime(ROLES, device="cpu", seed=7).evaluate_computation(
        _program(), {"i": INDEX, "t": TABLE}))


def test_parties_as_threads():
    rt = LocalMooseRuntime(ROLES, device_map={r: "cpu" for r in ROLES}, seed=7)
    _check_program(rt.evaluate_computation(_program(), {"i": INDEX, "t": TABLE}))


@pytest.mark.gpu
def test_parties_as_threads_on_a_device():
    rt = LocalMooseRuntime(ROLES, device_map={r: "cuda:0" for r in ROLES}, seed=7)
    _check_program(rt.evaluate_computation(_program(), {"i": INDEX, "t": TABLE}))


@pytest.mark.parametrize("ring", [64, 128])
def test_lowered_graph_takes_no_new_operator_and_agrees(ring):
    low = passes.compile(to_native(_program(ring), ring),
                         arg_specs={"i": INDEX.shape, "t": TABLE.shape}, fixedpoint_ring=ring)
    assert passes.is_lowered(low)
    passes.well_formed(low)
    kinds = {o.kind for o in low.operations}
    assert not kinds & {"OneHot", "Lookup", "BinCount", "OuterCross", "Demux"}
    parent = passes.compile(to_native(_parent_program(ring), ring),
                            arg_specs={"i": INDEX.shape, "t": TABLE.shape}, fixedpoint_ring=ring)
    assert kinds <= {o.kind for o in parent.operations}  # only leaf operators that existed
    txt = low.to_textual()
    again = Computation.from_textual(txt)
    assert again.to_textual() == txt
    out = LocalMooseRuntime(ROLES, device="cpu", fixedpoint_ring=ring).evaluate_compiled(
        again, {"i": INDEX, "t": TABLE})
    _check_program(out)


def _parent_program(ring):
    """A program of operators older than the demultiplexer whose lowering uses every leaf
    operator a lowered lookup may: a sort, a group-by, a dot, an argmax, a broadcast."""
    dt = {64: pm.fixed(14, 23), 128: pm.fixed(24, 40)}[ring]

    @pm.computation
    def prog(i: pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64), shape=INDEX.shape),
             t: pm.Argument(placement=BOB, vtype=pm.TensorType(pm.float64), shape=TABLE.shape)):
        with ALICE:
            x = pm.cast(i, dtype=dt)
        with BOB:
            tf = pm.cast(t, dtype=dt)
        with REP:
            outs = (pm.group_by_sum(tf, by=0, shuffle=False), pm.dot(pm.transpose(tf), tf),
                    pm.mul(pm.expand_dims(x, 1), pm.expand_dims(x, 0)),
                    pm.argmax(tf, axis=0, upmost_index=33), pm.sum(tf, 0), pm.sigmoid(x))
        with CAROLE:
            return tuple(pm.cast(o, dtype=pm.float64) for o in outs)

    return prog
