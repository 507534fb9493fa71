"""fixedpoint.sort on a seeded stacked session: the revealed ring values are numpy's sort of the
encoded integers exactly (nothing truncates), for plain sorts along any axis, both orders and
padded lengths, and for rows ordered by a key column; the dtype bound; the number of sign
extractions of the network."""
import numpy as np
import pytest

from moose_amd.ir.computation import ReplicatedPlacement
from moose_amd.ops import ring as R
from moose_amd.protocols import fixedpoint as fxp
from moose_amd.protocols import replicated as rep
from moose_amd.runtime.session import HV
from moose_amd.runtime.session import StackedSession

PLC = ReplicatedPlacement(("a", "b", "c"))
DTYPES = {64: (14, 23), 128: (24, 40)}  # fixed(14, 23) over Z_2^64, fixed(24, 40) over Z_2^128
DEVICES = ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)]
LENGTHS = (1, 2, 3, 5, 8, 33)


def _shared(sess, vals, bits, device):
    integ, frac = DTYPES[bits]
    enc = np.vectorize(lambda v: int(v) % (1 << bits), otypes=[object])(vals)
    t = rep.share(sess, PLC, HV("a", R.from_ints(enc, bits, device)))
    return fxp.RepFixed(t, frac, integ)


def _revealed(sess, x):
    return R.to_signed_ints(R.RT(rep.reveal(sess, x.t, "c").v.data.cpu(), x.bits))


def _values(rng, shape, bits):
    """Encoded integers with duplicates, negatives and the extremes +-(2^i - 2^-f)."""
    integ, frac = DTYPES[bits]
    top = (1 << (integ + frac)) - 1
    n = int(np.prod(shape))
    vals = [int(v) for v in rng.integers(-(1 << 36), 1 << 36, size=n)]  # inside both types
    pool = [top, -top, 0, -1, vals[0], vals[0]]
    for i, v in zip(rng.permutation(n), pool):
        vals[i] = v
    return np.array(vals, dtype=object).reshape(shape)


def _np_sort(vals, axis, descending):
    s = np.sort(vals, axis=axis)
    return np.flip(s, axis=axis) if descending else s


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("n", LENGTHS)
def test_sort_equals_numpy_exactly(device, bits, n):
    sess = StackedSession(device, seed=5)
    rng = np.random.default_rng(100 * bits + n)
    for shape, axis in (((3, n), -1), ((n, 2), 0)):  # the last axis, and one that is not
        vals = _values(rng, shape, bits)
        x = _shared(sess, vals, bits, device)
        for descending in (False, True):
            got = _revealed(sess, fxp.sort(sess, x, axis=axis, descending=descending))
            assert got.shape == vals.shape
            assert (got == _np_sort(vals, axis, descending)).all(), (shape, axis, descending)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bits", [64, 128])
def test_sort_a_middle_axis(device, bits):
    sess = StackedSession(device, seed=6)
    vals = _values(np.random.default_rng(bits), (2, 5, 3), bits)
    got = _revealed(sess, fxp.sort(sess, _shared(sess, vals, bits, device), axis=1))
    assert (got == np.sort(vals, axis=1)).all()


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bits", [64, 128])
def test_sort_rows_by_a_key_column(device, bits):
    sess = StackedSession(device, seed=7)
    rng = np.random.default_rng(bits + 1)
    integ, frac = DTYPES[bits]
    inside = (1 << (integ + frac)) - 2  # the largest key strictly inside the type's range
    for by in (0, 2):
        a = _values(rng, (7, 3), bits)
        # distinct keys, the documented boundary among them: the order of the rows is determined
        a[:, by] = [int(v) for v in rng.permutation(7) * 1000 - 3000]
        a[2, by], a[5, by] = inside, -inside
        x = _shared(sess, a, bits, device)
        for descending in (False, True):
            got = _revealed(sess, fxp.sort(sess, x, by=by, descending=descending))
            order = sorted(range(7), key=lambda r: a[r, by], reverse=descending)
            assert (got == a[order]).all(), (by, descending)
    # duplicate keys: the multiset of rows is preserved and the key column is sorted
    a = _values(rng, (7, 3), bits)
    a[:, 1] = [5, -2, 5, 5, -2, 0, 7]
    got = _revealed(sess, fxp.sort(sess, _shared(sess, a, bits, device), by=1))
    assert [int(v) for v in got[:, 1]] == sorted(int(v) for v in a[:, 1])
    assert sorted(tuple(int(v) for v in r) for r in got) == \
        sorted(tuple(int(v) for v in r) for r in a)


def test_a_dtype_without_room_for_the_difference_is_refused():
    sess = StackedSession("cpu", seed=8)
    t = rep.share(sess, PLC, HV("a", R.from_ints(np.arange(4, dtype=object), 64, "cpu")))
    with pytest.raises(ValueError, match=r"integral \+ fractional \+ 2"):
        fxp.sort(sess, fxp.RepFixed(t, 23, 40))  # 40 + 23 + 2 = 65 bits over Z_2^64
    ok = fxp.sort(sess, fxp.RepFixed(t, 23, 39))  # 64 bits: the ring's own sign
    assert [int(v) for v in _revealed(sess, ok)] == [0, 1, 2, 3]
    with pytest.raises(ValueError, match="rank-2"):
        fxp.sort(sess, fxp.RepFixed(t, 23, 14), by=0)


@pytest.mark.parametrize("n,stages", [(8, 6), (33, 21)])
def test_number_of_sign_extractions(monkeypatch, n, stages):
    calls = []
    real = rep.less_than_zero_arith

    def counted(sess, x, width=None):
        calls.append(width)
        return real(sess, x, width=width)

    monkeypatch.setattr(rep, "less_than_zero_arith", counted)
    sess = StackedSession("cpu", seed=9)
    vals = _values(np.random.default_rng(n), (n,), 64)
    got = _revealed(sess, fxp.sort(sess, _shared(sess, vals, 64, "cpu")))
    assert (got == np.sort(vals)).all()
    assert len(calls) == stages
    assert set(calls) == {14 + 23 + 2}
