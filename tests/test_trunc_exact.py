"""What TruncPr must compute, as an integer model that shares no arithmetic with the kernels.

Probabilistic truncation is deterministic once the opening mask is known.  Over Z_2^W, for
-2^(W-2) <= x < 2^(W-2), the mask r = r0 + r1 (mod 2^W) and the arithmetic shift >>, the new
sharing reveals to

    y = (x >> m) + [(x mod 2^m) + (r mod 2^m) >= 2^m]      (mod 2^W)

with slots z0 = PRF(k0, nonce_z0), z2 = PRF(k2, nonce_z2), z1 = y - z0 - z2 and
out1[p] = out0[p + 1].  (c = x + 2^(W-2) + r is opened and ``ov`` is the carry of its low W-1
bits, so floor(x' / 2^m) = c_top - r_top + ov 2^(k-m) - [c mod 2^m < r mod 2^m].)

Every kernel that carries the protocol is pinned to this on the host and on the device: the
stacked TruncPr (mx_trunc_pr3 and its key-slot, row-view and premultiplied forms, both output
layouts, past the launch-grid cap), the fused product tail (mx_mul_trunc3_kv, two-job form),
the opened tail (mx_mul_trunc3_open), the polynomial tail (k_wsum_trunc3_lat) and the
per-party rounds (mx_trunc_party_r*, mx_dot_tail_r*).  The streams r0, r1, z0, z2 are read
with ``prf_expand``; inputs are chosen from the mask, never from a kernel's answer; every
comparison is exact.  The shift range of the entries (csrc/moosex.h) is pinned by return code.

Shifts: the opening and per-party entries accept 1..63, but TruncPr over Z_2^64 is defined up
to m = 62 only (2^(W-2) >> m must be an integer), so their cases are m in {1, 23, 63} over
Z_2^128 and {1, 23, 62} over Z_2^64.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from moose_amd.ir.computation import ReplicatedPlacement
from moose_amd.ops import native as nat
from moose_amd.ops import ring as R
from moose_amd.runtime import keys as K
from moose_amd.runtime.session import PV
from moose_amd.runtime.session import StackedSession
from test_party_rounds import SIZES as PARTY_SIZES

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
GPU = [pytest.param("cuda", marks=pytest.mark.gpu)]
PLC = ReplicatedPlacement(("alice", "bob", "carole"))
KEYS = [bytes(range(16)), bytes(range(50, 66)), bytes(range(100, 116))]  # k0, k1, k2
NMUL = 3000
NONCES = tuple(3001 + i for i in range(6))  # r0, r1, t, m, z0, z2
SHIFTS = {64: [0, 1, 23, 31, 32, 33, 61, 62], 128: [0, 1, 23, 63, 64, 65, 125, 126]}
NARROW = {64: [1, 23, 62], 128: [1, 23, 63]}  # entries that accept 1..63 (module doc)
FRAC = 23
# one ChaCha block of 4 chunks per thread, 2048 blocks of 256 threads (prf_dev.h grid_for)
CAP_CHUNKS = 4 * 2048 * 256
U = np.uint64


def _per(bits):
    return 2 if bits == 64 else 1  # elements per 16-byte keystream chunk


def _sizes(bits, lat_only=False):
    """The chunk tail, the 42-chunk blocks of the latency kernels, the last latency and first
    throughput size (8192 chunks) and a throughput launch of several workgroups."""
    lat = [1, 3, 4, 5, 255, 1023, 8192 * _per(bits)]
    return lat if lat_only else lat + [8192 * _per(bits) + 1, 70001]


# ---------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------
def model(x, r, m, W):
    """y of the module doc for one element: x signed, r unsigned, python integers."""
    low = (1 << m) - 1
    carry = ((x & low) + (r & low)) >> m  # the bracket: 0 or 1
    return ((x >> m) + carry) & ((1 << W) - 1)


def model_u64(x, r, m):
    """The same over Z_2^64 on numpy arrays: x int64, r uint64 -> uint64 (0 <= m <= 62, so
    the sum of the two low parts stays below 2^63)."""
    low = U((1 << m) - 1)
    carry = ((x.view(U) & low) + (r & low)) >> U(m)
    return (x >> np.int64(m)).view(U) + carry


# ---------------------------------------------------------------------------------------
# ring elements as numpy: Z_2^64 = uint64 [n], Z_2^128 = uint64 [n, 2] (lo, hi)
# ---------------------------------------------------------------------------------------
def _np(t):
    return t.detach().cpu().contiguous().numpy().view(U)


def _t(a, device="cpu"):
    """A tensor of its own: cached inputs are never handed to native code as aliases."""
    return torch.from_numpy(np.array(a, copy=True, order="C").view(np.int64)).to(device)


def _add(a, b, bits):
    if bits == 64:
        return a + b
    lo = a[..., 0] + b[..., 0]
    return np.stack([lo, a[..., 1] + b[..., 1] + (lo < a[..., 0]).astype(U)], -1)


def _neg(a, bits):
    if bits == 64:
        return U(0) - a
    one = np.zeros_like(a)
    one[..., 0] = 1
    return _add(~a, one, 128)


def _signed(a, bits):
    """Signed python integers (an object array) of ring elements."""
    if bits == 64:
        return a.view(np.int64).astype(object)
    return a[..., 0].astype(object) + a[..., 1].view(np.int64).astype(object) * (1 << 64)


def _ring(ints, bits):
    """Ring elements of python integers (reduced mod 2^bits)."""
    v = [int(i) % (1 << bits) for i in ints]
    if bits == 64:
        return np.array(v, dtype=U)
    return np.array([[i & (2**64 - 1), i >> 64] for i in v], dtype=U).reshape(len(v), 2)


def _uniform(rng, n, bits):
    return rng.integers(0, 2**64, (n,) if bits == 64 else (n, 2), dtype=U)


def _in_range(rng, n, bits, log2=None):
    """Uniform over -2^log2 <= x < 2^log2 (default: TruncPr's whole range, log2 = bits - 2)."""
    log2 = bits - 2 if log2 is None else log2
    if log2 <= 62:
        v = rng.integers(-(1 << log2), 1 << log2, n, dtype=np.int64).view(U)
        return v if bits == 64 else np.stack([v, (v.view(np.int64) >> np.int64(63)).view(U)], -1)
    hi = rng.integers(-(1 << (log2 - 64)), 1 << (log2 - 64), n, dtype=np.int64).view(U)
    return np.stack([rng.integers(0, 2**64, n, dtype=U), hi], -1)


def _edges(m, bits, limit=None):
    """0, +-1, the ends of the range, and the values around 2^m -- those inside the range
    (and below ``limit`` in magnitude)."""
    q = 1 << (bits - 2)
    e = [0, 1, -1, q - 1, -q, (1 << m) - 1, 1 << m, -(1 << m), (1 << m) + 1, -(1 << m) - 1]
    e = [v for v in dict.fromkeys(e) if -q <= v < q]
    return e if limit is None else [v for v in e if -limit <= v < limit]


def _values(n, m, bits, seed, log2=None):
    """The edge values, then seeded values uniform over the whole valid range (3 of 4) and over
    +-2^40 (1 of 4).  ``log2``: a narrower range for everything."""
    rng = np.random.default_rng(seed)
    wide = _in_range(rng, n, bits, log2)
    small = _in_range(rng, n, bits, min(40, bits - 2 if log2 is None else log2))
    v = np.where((np.arange(n) % 4 == 3).reshape((n,) + (1,) * (wide.ndim - 1)), small, wide)
    e = _edges(m, bits, None if log2 is None else 1 << log2)[:n]
    v[:len(e)] = _ring(e, bits)
    return v


def _share(v, bits, seed):
    """[3, n] slots of the values: x0, x1 uniform, x2 = v - x0 - x1."""
    rng = np.random.default_rng(seed)
    x0, x1 = _uniform(rng, len(v), bits), _uniform(rng, len(v), bits)
    return np.stack([x0, x1, _add(v, _neg(_add(x0, x1, bits), bits), bits)])


@functools.lru_cache(maxsize=64)
def _stream(key_index, nonce, n, bits):
    """PRF(k, nonce) of n elements, as the kernels draw it."""
    return _np(R.prf_expand([KEYS[key_index]], nonce, (n,), bits, "cpu").data[0])


def _mask(n, bits, nonces=NONCES):
    return _add(_stream(0, nonces[0], n, bits), _stream(2, nonces[1], n, bits), bits)


def _expected(v, r, m, bits):
    """The model on arrays: numpy over Z_2^64, python integers over Z_2^128."""
    if bits == 64:
        return model_u64(v.view(np.int64), r, m)
    ru = r[..., 0].astype(object) + r[..., 1].astype(object) * (1 << 64)
    return _ring([model(int(x), int(q), m, 128) for x, q in zip(_signed(v, 128), ru)], 128)


def _coverage(v, r, m, bits):
    """From the inputs and the mask alone: the (r_msb, c_msb) combinations of the opening
    c = x + 2^(W-2) + r, and the values the bracket takes."""
    q = _ring([1 << (bits - 2)] * len(v), bits)
    c = _add(_add(v, q, bits), r, bits)
    top = (lambda a: a >> U(63)) if bits == 64 else (lambda a: a[..., 1] >> U(63))
    combos = set(zip(top(r).tolist(), top(c).tolist()))
    if bits == 64:
        low = U((1 << m) - 1)
        carry = set((((v & low) + (r & low)) >> U(m)).tolist())
    else:
        low = (1 << m) - 1
        carry = {((int(x) & low) + (int(y) & low)) >> m
                 for x, y in zip(_signed(v, 128), _signed(r, 128))}
    return combos, carry


def _assert_coverage(v, r, m, bits, edges=None):
    """Issue conditions for a case of n >= 255: every mask case, both bracket values (m = 0
    has no low part: the bracket is 0), every edge value."""
    if len(v) < 255:
        return
    combos, carry = _coverage(v, r, m, bits)
    assert combos == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert carry == ({0, 1} if m else {0})
    have = set(_signed(v, bits).tolist())
    assert all(e in have for e in (_edges(m, bits) if edges is None else edges))


@functools.lru_cache(maxsize=None)
def _case(bits, m, n, nonces=NONCES):
    """(values, slots, expected reveal) of one stacked case: computed once, never written."""
    v = _values(n, m, bits, seed=1000 * m + n)
    r = _mask(n, bits, nonces)
    _assert_coverage(v, r, m, bits)
    return v, _share(v, bits, n + 1), _expected(v, r, m, bits)


def _check(out0, out1, want, bits, nonces=NONCES, add0=None):
    """Assertions 1-3 on the two [3, n] share vectors (tensors).  ``add0``: a public constant
    that the entry adds to party 0's slot."""
    o0, o1 = _np(out0), _np(out1)
    n = o0.shape[1]
    z0, z2 = _stream(0, nonces[4], n, bits), _stream(2, nonces[5], n, bits)
    if add0 is not None:
        z0 = _add(z0, _ring([add0] * n, bits), bits)
        want = _add(want, _ring([add0] * n, bits), bits)
    assert np.array_equal(o0[0], z0) and np.array_equal(o0[2], z2)
    for p in range(3):
        assert np.array_equal(o1[p], o0[(p + 1) % 3]), p
    assert np.array_equal(_add(_add(o0[0], o0[1], bits), o0[2], bits), want)


# ---------------------------------------------------------------------------------------
# calling the entries
# ---------------------------------------------------------------------------------------
_SLOTS = {}


def _key_slots(device):
    """Three consecutive key slots k0, k1, k2 in the memory of ``device``."""
    if device not in _SLOTS:
        _SLOTS[device] = torch.from_numpy(K.slot_words(KEYS).view(np.int32).copy()).to(device)
    return _SLOTS[device]


def _slot(device, i):
    return _key_slots(device)[i].data_ptr()


def _nn(nonces):
    return (ctypes.c_uint64 * len(nonces))(*nonces)


def _outputs(n, bits, device, aliased):
    out = (R.ring4 if aliased else R.empty2)((3, n), bits, device)
    w = bits // 8
    assert (out[1].data.data_ptr() == out[0].data.data_ptr() + w * n) == aliased
    return out[0].data, out[1].data


def _sync(device):
    if device != "cpu":
        torch.cuda.synchronize()


def _trunc_pr3(entry, s0, m, bits, device, aliased=True, nonces=NONCES):
    """mx_trunc_pr3 (raw keys) / mx_trunc_pr3_k (key slots) on [3, n] slots."""
    d = _t(s0, device)
    n = s0.shape[1]
    o0, o1 = _outputs(n, bits, device, aliased)
    if entry == "raw":
        keys = [ctypes.create_string_buffer(KEYS[i], 16) for i in (0, 2)]
        fn = nat.lib().mx_trunc_pr3
    else:
        keys = [_slot(device, 0), _slot(device, 2)]
        fn = nat.lib().mx_trunc_pr3_k
    rc = fn(nat.dev_of(d), bits // 64, nat.ptr(d), nat.ptr(o0), nat.ptr(o1), n, m, *keys,
            _nn(nonces), nat.stream_of(d))
    _sync(device)
    assert rc == 0
    return o0, o1


# ---------------------------------------------------------------------------------------
# the model's two forms agree
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", SHIFTS[64])
def test_numpy_form_of_the_model_is_the_integer_form(m):
    v, r = _values(1023, m, 64, seed=m), _mask(1023, 64)
    want = [model(int(x), int(q), m, 64) for x, q in zip(v.view(np.int64), r)]
    assert model_u64(v.view(np.int64), r, m).tolist() == want


def test_model_is_floor_or_floor_plus_one():
    """The error of the truncation is the bracket: 0 or 1 above floor(x / 2^m)."""
    for bits in (64, 128):
        for m in SHIFTS[bits]:
            v, r = _values(255, m, bits, seed=m), _mask(255, bits)
            for x, y in zip(_signed(v, bits), _signed(_expected(v, r, m, bits), bits)):
                assert y - (x >> m) in ((0, 1) if m else (0,))


# ---------------------------------------------------------------------------------------
# stacked TruncPr
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("bits,m", [(b, m) for b in (64, 128) for m in SHIFTS[b]])
def test_stacked_trunc_pr_reveals_the_model(dev, bits, m):
    for i, n in enumerate(_sizes(bits)):
        _, s0, want = _case(bits, m, n)
        # raw keys / key slots and the two output layouts, in turn over the sizes
        entry, aliased = ("raw", "k")[i % 2], (i // 2) % 2 == 0
        _check(*_trunc_pr3(entry, s0, m, bits, dev, aliased), want, bits)
        if n in (5, 1023):
            _check(*_trunc_pr3("raw" if entry == "k" else "k", s0, m, bits, dev, not aliased),
                   want, bits)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("bits", [64, 128])
def test_session_fused_trunc_pr_reveals_the_model(dev, bits):
    """Through StackedSession.fused_trunc_pr, on the session's own keys."""
    from moose_amd.protocols import replicated as rep

    sess = StackedSession(dev, seed=11)
    base = sess.setup(PLC)
    k0, k2 = sess.keytable.raw_key(base), sess.keytable.raw_key(base + 2)
    m, n = 23, 1023
    v, s0, _ = _case(bits, m, n)
    d = _t(s0, dev)
    x = rep.RepTensor(PLC, bits, "arith", PV(PLC, R.RT(d, bits)),
                      PV(PLC, R.RT(torch.roll(d, -1, 0).contiguous(), bits)))
    t0, t1 = sess.fused_trunc_pr(x, m, NONCES)
    _sync(dev)
    draw = lambda k, nc: _np(R.prf_expand([k], nc, (n,), bits, "cpu").data[0])  # noqa: E731
    r = _add(draw(k0, NONCES[0]), draw(k2, NONCES[1]), bits)
    _assert_coverage(v, r, m, bits)  # on the session's mask, not the module keys'
    o0, o1 = _np(t0.v.data), _np(t1.v.data)
    assert np.array_equal(o0[0], draw(k0, NONCES[4])) and np.array_equal(o0[2], draw(k2, NONCES[5]))
    assert all(np.array_equal(o1[p], o0[(p + 1) % 3]) for p in range(3))
    assert np.array_equal(_add(_add(o0[0], o0[1], bits), o0[2], bits), _expected(v, r, m, bits))


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("bits,m", [(b, m) for b in (64, 128) for m in SHIFTS[b]])
def test_trunc_pr_row_views_leave_the_rest_of_the_stack_alone(dev, bits, m):
    """mx_trunc_pr3_ko: the party slots are rows of a larger prefilled stack."""
    fill = 0x5A5A5A5A5A5A5A5A
    w = bits // 64
    for n in _sizes(bits):
        total, at = n + 40, 17
        _, s0, want = _case(bits, m, n)
        d = _t(s0, dev)
        big = [torch.full((3, total * w), fill, dtype=torch.int64, device=dev) for _ in range(2)]
        o0, o1 = (b[:, at * w:(at + n) * w] for b in big)
        rc = nat.lib().mx_trunc_pr3_ko(
            nat.dev_of(d), w, nat.ptr(d), o0.data_ptr(), o1.data_ptr(), n, m, _slot(dev, 0),
            _slot(dev, 2), _nn(NONCES), total, nat.stream_of(d))
        _sync(dev)
        assert rc == 0
        shp = (3, n, 2) if bits == 128 else (3, n)
        _check(o0.reshape(shp), o1.reshape(shp), want, bits)
        for b in big:
            assert bool((b[:, :at * w] == fill).all()) and bool((b[:, (at + n) * w:] == fill).all())


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("cm", [1, 3, -1])
@pytest.mark.parametrize("bits,m", [(b, m) for b in (64, 128) for m in SHIFTS[b]])
def test_premultiplied_trunc_pr_reveals_the_model_of_cm_x(dev, bits, m, cm):
    """mx_trunc_pr3_kmo with cm in {1, 3, 2^W - 1}: the shared x is chosen so that cm * x is
    the in-range value t the model takes (3 (t div 3), or -(-t)).  Of the edge values only the
    multiples of 3 can be 3 x."""
    edges = [e for e in _edges(m, bits) if cm != 3 or e % 3 == 0]
    for n in _sizes(bits):
        t, r = _values(n, m, bits, seed=7 * m + n), _mask(n, bits)
        if cm == 3:
            x = _ring([int(i) // 3 for i in _signed(t, bits)], bits)
            t = _ring([3 * (int(i) // 3) for i in _signed(t, bits)], bits)
        else:
            x = t if cm == 1 else _neg(t, bits)
        _assert_coverage(t, r, m, bits, edges=edges)
        d = _t(_share(x, bits, n), dev)
        o0, o1 = _outputs(n, bits, dev, aliased=n % 2 == 1)
        c = cm % (1 << bits)
        rc = nat.lib().mx_trunc_pr3_kmo(
            nat.dev_of(d), bits // 64, nat.ptr(d), nat.ptr(o0), nat.ptr(o1), n, m,
            _slot(dev, 0), _slot(dev, 2), _nn(NONCES), n,
            (ctypes.c_uint64 * 2)(c & (2**64 - 1), c >> 64), nat.stream_of(d))
        _sync(dev)
        assert rc == 0
        _check(o0, o1, _expected(t, r, m, bits), bits)


@pytest.mark.gpu
def test_stacked_trunc_pr_past_the_grid_cap_z64():
    """The throughput kernel's grid-stride loop takes a second trip: checked in full."""
    bits, m, n = 64, 23, 2 * CAP_CHUNKS + 5
    rng = np.random.default_rng(5)
    v = _in_range(rng, n, bits)
    r = _add(_np(R.prf_expand([KEYS[0]], NONCES[0], (n,), bits, "cpu").data[0]),
             _np(R.prf_expand([KEYS[2]], NONCES[1], (n,), bits, "cpu").data[0]), bits)
    o0, o1 = _trunc_pr3("k", _share(v, bits, 6), m, bits, "cuda", aliased=True)
    for key, nonce, slot in ((0, NONCES[4], 0), (2, NONCES[5], 2)):
        assert torch.equal(o0[slot], R.prf_expand([KEYS[key]], nonce, (n,), bits, "cuda").data[0])
    for p in range(3):
        assert torch.equal(o1[p], o0[(p + 1) % 3])
    got = _np(o0)
    assert np.array_equal(got[0] + got[1] + got[2], model_u64(v.view(np.int64), r, m))


@pytest.mark.gpu
def test_stacked_trunc_pr_past_the_grid_cap_z128():
    """Over Z_2^128: the z0 / z2 slots in full against prf_expand on the device, the reveal with
    python integers at both ends, around the cap and at a stride of 4099 elements."""
    bits, m, n = 128, 65, CAP_CHUNKS + 5
    rng = np.random.default_rng(8)
    v = _in_range(rng, n, bits)
    o0, o1 = _trunc_pr3("k", _share(v, bits, 9), m, bits, "cuda", aliased=True)
    for key, nonce, slot in ((0, NONCES[4], 0), (2, NONCES[5], 2)):
        assert torch.equal(o0[slot], R.prf_expand([KEYS[key]], nonce, (n,), bits, "cuda").data[0])
    for p in range(3):
        assert torch.equal(o1[p], o0[(p + 1) % 3])
    idx = np.unique(np.concatenate([np.arange(64), np.arange(n - 64, n),
                                    np.arange(CAP_CHUNKS - 64, n),  # the cap: the second trip
                                    np.arange(0, n, 4099)]))
    r = _add(_np(R.prf_expand([KEYS[0]], NONCES[0], (n,), bits, "cpu").data[0])[idx],
             _np(R.prf_expand([KEYS[2]], NONCES[1], (n,), bits, "cpu").data[0])[idx], bits)
    got = _np(o0[:, torch.from_numpy(idx).cuda()])
    assert np.array_equal(_add(_add(got[0], got[1], bits), got[2], bits),
                          _expected(v[idx], r, m, bits))


# ---------------------------------------------------------------------------------------
# the fused product tail (device only: the host entry returns 1 and the caller composes)
# ---------------------------------------------------------------------------------------
def _factors(n, m, bits, seed):
    """x, y with |x y| < 2^(W-2): the edge values times +-1, then both uniform over half the
    width.  Returns (x, y, x y) as ring elements."""
    rng = np.random.default_rng(seed)
    half = bits // 2 - 2
    x, y = _in_range(rng, n, bits, half), _in_range(rng, n, bits, half)
    e = _edges(m, bits)
    q = 1 << (bits - 2)
    pairs = [(v, 1) for v in e] + [(v, -1) for v in e if -q <= -v < q]
    pairs = pairs[:n]
    x[:len(pairs)] = _ring([a for a, _ in pairs], bits)
    y[:len(pairs)] = _ring([b for _, b in pairs], bits)
    prod = _ring([int(a) * int(b) for a, b in zip(_signed(x, bits), _signed(y, bits))], bits)
    return x, y, prod


def _rep(slots, dev, bits):
    """(s0, s1) of a stacked replicated value: s1[p] = s0[p + 1]."""
    d = _t(slots, dev)
    return R.RT(d, bits), R.RT(torch.roll(d, -1, 0).contiguous(), bits)


@pytest.mark.parametrize("dev", GPU)
@pytest.mark.parametrize("bits,m", [(b, m) for b in (64, 128) for m in SHIFTS[b]])
def test_mul_trunc_with_operands_reveals_the_model_of_the_product(dev, bits, m):
    for n in _sizes(bits):
        x, y, prod = _factors(n, m, bits, seed=3 * m + n)
        r = _mask(n, bits)
        _assert_coverage(prod, r, m, bits, edges=[e for e in _edges(m, bits)])
        x0, x1 = _rep(_share(x, bits, 1), dev, bits)
        y0, y1 = _rep(_share(y, bits, 2), dev, bits)
        out = R.mul_trunc3_k(x0, x1, y0, y1, _slot(dev, 0), NMUL, m, NONCES)
        _sync(dev)
        _check(out[0].data, out[1].data, _expected(prod, r, m, bits), bits)


@pytest.mark.parametrize("dev", GPU)
@pytest.mark.parametrize("bits,m", [(b, m) for b in (64, 128) for m in SHIFTS[b]])
def test_mul_trunc_with_the_product_given_reveals_the_model(dev, bits, m):
    for n in _sizes(bits):
        _, s0, want = _case(bits, m, n)
        out = R.zs_trunc3_k(R.RT(_t(s0, dev), bits), _slot(dev, 0), NMUL, m, NONCES)
        _sync(dev)
        _check(out[0].data, out[1].data, want, bits)


@pytest.mark.parametrize("dev", GPU)
@pytest.mark.parametrize("bits", [64, 128])
def test_mul_trunc_reads_strided_operand_views(dev, bits):
    m, n = 23, 1023
    x, y, prod = _factors(n, m, bits, seed=77)
    _assert_coverage(prod, _mask(n, bits), m, bits)
    w = bits // 64

    def view(t, pad):
        big = torch.zeros((3, (n + pad) * w), dtype=torch.int64, device=dev)
        big[:, 5 * w:(5 + n) * w] = t.data.reshape(3, n * w)
        v = big[:, 5 * w:(5 + n) * w]
        v = v.reshape(3, n, 2) if bits == 128 else v
        assert not v.is_contiguous()
        return R.RT(v, bits)

    x0, x1 = _rep(_share(x, bits, 1), dev, bits)
    y0, y1 = _rep(_share(y, bits, 2), dev, bits)
    out = R.mul_trunc3_k(view(x0, 9), view(x1, 30), view(y0, 11), y1, _slot(dev, 0), NMUL, m,
                         NONCES)
    _sync(dev)
    _check(out[0].data, out[1].data, _expected(prod, _mask(n, bits), m, bits), bits)


@pytest.mark.parametrize("dev", GPU)
@pytest.mark.parametrize("bits", [64, 128])
def test_two_job_mul_trunc_reveals_the_model_job_by_job(dev, bits):
    other = tuple(4001 + i for i in range(6))
    for (na, ma), (nb, mb) in (((5, SHIFTS[bits][1]), (1023, SHIFTS[bits][-1])),
                               ((8192 * _per(bits), SHIFTS[bits][4]), (255, 0))):
        jobs, wants = [], []
        for n, m, nmul, nonces in ((na, ma, NMUL, NONCES), (nb, mb, NMUL + 500, other)):
            x, y, prod = _factors(n, m, bits, seed=n + m)
            _assert_coverage(prod, _mask(n, bits, nonces), m, bits)
            x0, x1 = _rep(_share(x, bits, 1), dev, bits)
            y0, y1 = _rep(_share(y, bits, 2), dev, bits)
            jobs.append((x0, x1, y0, y1, nmul, m, nonces, None))
            wants.append((_expected(prod, _mask(n, bits, nonces), m, bits), nonces))
        outs = R.mul_trunc3_k2(jobs, _slot(dev, 0))
        _sync(dev)
        for (o0, o1), (want, nonces) in zip(outs, wants):
            _check(o0.data, o1.data, want, bits, nonces)


# ---------------------------------------------------------------------------------------
# the opened tail: out = float(signed(model)) / 2^frac, exact while |model| < 2^53
# ---------------------------------------------------------------------------------------
def _open_case(bits, m, n):
    log2 = min(bits - 2, 52 + m)
    v = _values(n, m, bits, seed=31 * m + n, log2=log2)
    r = _mask(n, bits)
    if n >= 255:
        _assert_coverage(v, r, m, bits, edges=_edges(m, bits, 1 << log2))
    y = _signed(_expected(v, r, m, bits), bits)
    assert all(abs(int(i)) < 1 << 53 for i in y)
    return v, np.array([float(int(i)) / 2**FRAC for i in y], dtype=np.float64)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("bits,m", [(b, m) for b in (64, 128) for m in NARROW[b]])
def test_opened_tail_is_the_decoded_model(dev, bits, m):
    for n in _sizes(bits):
        v, want = _open_case(bits, m, n)
        z = R.RT(_t(_share(v, bits, n), dev), bits)
        got = R.zs_trunc3_open(z, _slot(dev, 0), NMUL, m, NONCES, FRAC)
        _sync(dev)
        assert got.dtype == torch.float64 and tuple(got.shape) == (n,)
        assert np.array_equal(got.cpu().numpy().view(np.int64), want.view(np.int64)), (m, n)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("bits", [64, 128])
def test_opened_tail_reads_rows_of_a_larger_stack(dev, bits):
    m, rows, cols = 23, 41, 25
    n = rows * cols
    v, want = _open_case(bits, m, n)
    d = _t(_share(v, bits, n), dev).reshape((3, rows, cols) + ((2,) if bits == 128 else ()))
    big = torch.zeros((3, 2 * rows) + tuple(d.shape[2:]), dtype=torch.int64, device=dev)
    big[:, 7:7 + rows] = d
    view = R.RT(big[:, 7:7 + rows], bits)
    assert not view.data.is_contiguous()
    got = R.zs_trunc3_open(view, _slot(dev, 0), NMUL, m, NONCES, FRAC)
    _sync(dev)
    assert tuple(got.shape) == (rows, cols)
    assert np.array_equal(got.cpu().numpy().reshape(-1).view(np.int64), want.view(np.int64))


# ---------------------------------------------------------------------------------------
# the polynomial tail: TruncPr of a public weighted sum, plus a public constant on party 0
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", GPU)
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("bits", [64, 128])
def test_weighted_sum_tail_reveals_the_model_of_the_sum(dev, bits, rows):
    """k_wsum_trunc3_lat through StackedSession.p_wsum_trunc_add.  The rows other than the first
    are uniform ring elements and the first is solved for (the first weight is odd), so the
    weighted sum is the in-range value the model takes.  The session composes the three steps
    at m = 0, so that shift goes to the entry (mxh_wsum_trunc3) directly, on the same keys."""
    weights = [3, -2, 5][:rows]
    mask = (1 << bits) - 1
    cadd = 0x1234567 if bits == 64 else (1 << 100) + 77
    cases = [(m, 1023) for m in SHIFTS[bits]] + [(23, n) for n in _sizes(bits, lat_only=True)]
    for m, n in cases:
        sess = StackedSession(dev, seed=m + n)
        base = sess.setup(PLC)
        k0, k2 = sess.keytable.raw_key(base), sess.keytable.raw_key(base + 2)
        nonces = tuple(range(1, 7))  # a fresh session's first six draws
        draw = lambda k, nc: _np(R.prf_expand([k], nc, (n,), bits, "cpu").data[0])  # noqa: E731
        t = _values(n, m, bits, seed=n + m)
        r = _add(draw(k0, nonces[0]), draw(k2, nonces[1]), bits)
        _assert_coverage(t, r, m, bits)
        rng = np.random.default_rng(n)
        vals = [None] + [_uniform(rng, n, bits) for _ in range(rows - 1)]
        rest = sum((w * _signed(vals[k], bits) for k, w in enumerate(weights) if k),
                   np.zeros(n, dtype=object))
        inv = pow(weights[0], -1, 1 << bits)
        vals[0] = _ring([((int(ti) - ri) * inv) & mask for ti, ri in zip(_signed(t, bits), rest)],
                        bits)
        S = np.stack([_share(v, bits, 40 + k) for k, v in enumerate(vals)], 1)  # [3, rows, n]
        d = _t(S, dev)
        if m:
            got = sess.p_wsum_trunc_add(PLC, PV(PLC, R.RT(d, bits)), weights, m, cadd)
            assert got is not None
            o0, o1 = got[0].v.data, got[1].v.data
        else:
            o0, o1 = _outputs(n, bits, dev, aliased=True)
            wt = R.const_ints([w % (1 << bits) for w in weights], bits, dev)
            rc = nat.lib().mxh_wsum_trunc3(
                bits // 64, nat.ptr(d), rows * n, n, rows, nat.ptr(wt.data), nat.ptr(o0),
                nat.ptr(o1), n, m, sess.key_ptr(PLC, 0), sess.key_ptr(PLC, 2), _nn(nonces),
                (ctypes.c_uint64 * 2)(cadd & (2**64 - 1), cadd >> 64), nat.stream_of(d))
            assert rc == 0
        _sync(dev)
        o0, o1 = _np(o0), _np(o1)
        add = _ring([cadd] * n, bits)
        assert np.array_equal(o0[0], _add(draw(k0, nonces[4]), add, bits))  # cadd: out0 slot 0
        assert np.array_equal(o1[2], o0[0])  # ... and out1 slot 2
        assert np.array_equal(o0[2], draw(k2, nonces[5]))
        assert np.array_equal(o1[0], o0[1]) and np.array_equal(o1[1], o0[2])
        total = _add(_add(o0[0], o0[1], bits), o0[2], bits)
        assert np.array_equal(total, _add(_expected(t, r, m, bits), add, bits)), (m, n)


# ---------------------------------------------------------------------------------------
# per-party rounds: P0 and P1 exchange msg, P1 receives the dealer's rt1 and rm1, then w0 and
# w1 are exchanged and z1 = w0 + w1 (csrc/moosex.h)
# ---------------------------------------------------------------------------------------
ROLES = [[0, 1, 2], [1, 2, 0]]
NONCES7 = (NMUL,) + NONCES  # the dot tail's: zero share first


def _party_slots(roles, device):
    """Key-slot addresses of stacked components: one in role r holds (own k_r, next k_{r+1})."""
    return [_slot(device, k % 3) for r in roles for k in (r, r + 1)]


def _party_check(out0, out1, roles, want, bits):
    """The parties' final shares (component c in role roles[c] holds z_r, z_{r+1}), brought
    into party order, are a replicated sharing that reveals to the model."""
    c = {r: i for i, r in enumerate(roles)}
    _check(torch.stack([out0[c[p]].cpu() for p in range(3)]),
           torch.stack([out1[c[p]].cpu() for p in range(3)]), want, bits)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("roles", ROLES, ids=str)
@pytest.mark.parametrize("bits,n", PARTY_SIZES)
def test_trunc_party_rounds_reveal_the_model(dev, bits, n, roles):
    c = {r: i for i, r in enumerate(roles)}
    slots = _party_slots(roles, dev)
    for m in NARROW[bits]:
        _, x, want = _case(bits, m, n)
        s0 = R.RT(_t(np.stack([x[r] for r in roles]), dev), bits)
        s1 = R.RT(_t(np.stack([x[(r + 1) % 3] for r in roles]), dev), bits)
        msg, msg_rm, out0, out1 = R.trunc_party_r0(s0, s1, m, roles, slots, NONCES)
        rmk, rrt, rrm = torch.zeros_like(msg), torch.zeros_like(msg), torch.zeros_like(msg_rm)
        rmk[c[0]], rmk[c[1]] = msg[c[1]], msg[c[0]]
        rrt[c[1]], rrm[c[1]] = msg[c[2]], msg_rm[c[2]]
        w = R.trunc_party_r1(msg, rmk, rrt, rrm, out0, out1, bits, m, roles, slots, NONCES)
        _sync(dev)
        z1 = _t(_add(_np(w[c[0]]), _np(w[c[1]]), bits), dev)
        out1[c[0]], out0[c[1]] = z1, z1
        _party_check(out0, out1, roles, want, bits)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("roles", ROLES, ids=str)
@pytest.mark.parametrize("bits,n", PARTY_SIZES)
def test_dot_tail_rounds_reveal_the_model(dev, bits, n, roles):
    """The parties' local products are an additive sharing of x; P2's zero-masked product goes
    to P0 and P1 with the first round, and round 2 adds w0 + w1."""
    c = {r: i for i, r in enumerate(roles)}
    slots = _party_slots(roles, dev)
    for m in NARROW[bits]:
        _, x, want = _case(bits, m, n)
        cross = [_t(x[r], dev) for r in roles]
        out0 = [torch.zeros_like(t) for t in cross]
        out1 = [torch.zeros_like(t) for t in cross]
        msg, rt, rm = R.dot_tail_r0(cross, bits, m, roles, slots, NONCES7, out0, out1, n)
        pick = lambda at: [at.get(r) for r in roles]  # noqa: E731 - by role
        rmk = pick({0: msg[c[1]], 1: msg[c[0]]})
        rz = pick({0: msg[c[2]], 1: msg[c[2]]})
        rrt, rrm = pick({1: rt[c[2]]}), pick({1: rm[c[2]]})
        w = R.dot_tail_r1(msg, rmk, rz, rrt, rrm, bits, m, roles, slots, NONCES7, out0, out1, n)
        R.dot_tail_r2(w, pick({0: w[c[1]], 1: w[c[0]]}),
                      pick({0: out1[c[0]], 1: out0[c[1]]}), bits, roles, n)
        _sync(dev)
        _party_check(out0, out1, roles, want, bits)


# ---------------------------------------------------------------------------------------
# the shift range, by return code: a refused call launches nothing
# ---------------------------------------------------------------------------------------
def _entries(dev, bits):
    """name -> (call(m) -> return code, accepted shifts as (lowest, highest))."""
    w, lib = bits // 64, nat.lib()
    shp = (3, 1, 2) if bits == 128 else (3, 1)
    buf = lambda s=shp: torch.zeros(s, dtype=torch.int64, device=dev)  # noqa: E731
    s0, o0, o1, f = buf(), buf(), buf(), torch.zeros(1, dtype=torch.float64, device=dev)
    d, st = nat.dev_of(s0), nat.stream_of(s0)
    k0, k2, nn = _slot(dev, 0), _slot(dev, 2), _nn(NONCES)
    raw = [ctypes.create_string_buffer(KEYS[i], 16) for i in (0, 2)]
    one = (ctypes.c_uint64 * 2)(1, 0)
    P, I, U2 = ctypes.c_void_p * 2, ctypes.c_int64 * 2, ctypes.c_uint64 * 2
    wide = (0, bits - 2)
    narrow = (1, min(63, bits - 2))  # the check is 1..63; run only what TruncPr defines
    calls = {
        "mx_trunc_pr3": (lambda m: lib.mx_trunc_pr3(
            d, w, s0.data_ptr(), o0.data_ptr(), o1.data_ptr(), 1, m, *raw, nn, st), wide),
        "mx_trunc_pr3_k": (lambda m: lib.mx_trunc_pr3_k(
            d, w, s0.data_ptr(), o0.data_ptr(), o1.data_ptr(), 1, m, k0, k2, nn, st), wide),
        "mx_trunc_pr3_ko": (lambda m: lib.mx_trunc_pr3_ko(
            d, w, s0.data_ptr(), o0.data_ptr(), o1.data_ptr(), 1, m, k0, k2, nn, 1, st), wide),
        "mx_trunc_pr3_kmo": (lambda m: lib.mx_trunc_pr3_kmo(
            d, w, s0.data_ptr(), o0.data_ptr(), o1.data_ptr(), 1, m, k0, k2, nn, 1, one, st),
            wide),
        "mx_mul_trunc3_open": (lambda m: lib.mx_mul_trunc3_open(
            d, w, s0.data_ptr(), 1, f.data_ptr(), 1, k0, NMUL, m, nn, FRAC, st, None), narrow),
    }
    roles, pslots = R._roles_arr([0, 1, 2]), R._slots_arr(_party_slots([0, 1, 2], dev))
    rm = buf((3, 1))
    vp = lambda t: (ctypes.c_void_p * 3)(*[t[i].data_ptr() for i in range(3)])  # noqa: E731
    nn7 = _nn(NONCES7)
    calls.update({
        "mx_trunc_party_r0": (lambda m: lib.mx_trunc_party_r0(
            d, w, 1, m, 3, roles, s0.data_ptr(), s0.data_ptr(), o0.data_ptr(), rm.data_ptr(),
            o1.data_ptr(), o1.data_ptr(), pslots, nn, st), narrow),
        "mx_trunc_party_r1": (lambda m: lib.mx_trunc_party_r1(
            d, w, 1, m, 3, roles, s0.data_ptr(), s0.data_ptr(), s0.data_ptr(), rm.data_ptr(),
            o0.data_ptr(), o1.data_ptr(), o1.data_ptr(), pslots, nn, st), narrow),
        "mx_dot_tail_r0": (lambda m: lib.mx_dot_tail_r0(
            d, w, 1, m, 3, roles, vp(s0), vp(o0), vp(o0), vp(rm), vp(o1), vp(o1), pslots, nn7,
            st), narrow),
        "mx_dot_tail_r1": (lambda m: lib.mx_dot_tail_r1(
            d, w, 1, m, 3, roles, vp(s0), vp(s0), vp(s0), vp(s0), vp(rm), vp(o0), vp(o1), vp(o1),
            pslots, nn7, st), narrow),
    })
    # the device-only entries refuse a shift on the host side, before anything is launched;
    # an accepted one is only run where there is a device
    calls["mx_mul_trunc3_kv"] = (lambda m: lib.mx_mul_trunc3_kv(
        d, w, s0.data_ptr(), None, None, None, o0.data_ptr(), o1.data_ptr(), 1, 1, k0, NMUL, m,
        nn, None, st), wide if d else None)
    p2 = lambda t: P(t.data_ptr(), t.data_ptr())  # noqa: E731
    nul = P(None, None)
    calls["mxh_mul_trunc3_kv2"] = (lambda m: lib.mxh_mul_trunc3_kv2(
        w, p2(s0), nul, nul, nul, p2(o0), p2(o1), I(1, 1), I(1, 1), k0, U2(NMUL, NMUL),
        (ctypes.c_int * 2)(1, m), _nn(NONCES + NONCES), nul, st), wide if d else None)
    calls["mxh_mul_trunc3_kv2 (first job)"] = (lambda m: lib.mxh_mul_trunc3_kv2(
        w, p2(s0), nul, nul, nul, p2(o0), p2(o1), I(1, 1), I(1, 1), k0, U2(NMUL, NMUL),
        (ctypes.c_int * 2)(m, 1), _nn(NONCES + NONCES), nul, st), wide if d else None)
    S, wt = buf((3, 1) + shp[1:]), buf(shp[1:])
    calls["mxh_wsum_trunc3"] = (lambda m: lib.mxh_wsum_trunc3(
        w, S.data_ptr(), 1, 1, 1, wt.data_ptr(), o0.data_ptr(), o1.data_ptr(), 1, m, k0, k2, nn,
        one, st), wide if d else None)
    return calls


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("bits", [64, 128])
def test_shift_range_by_return_code(dev, bits):
    """Stacked entries: 0 <= m <= W - 2; opening and per-party entries: 1 <= m <= 63.  Anything
    else is -3 on the host and on the device (valid 1-element buffers: a refused call launches
    nothing).  The ends of the stacked range are accepted; of 1..63, the ends that TruncPr
    defines over the ring are run (over Z_2^64 that is 62: m = 63 is accepted there, and its
    result undefined, so the protocol entries refuse it first)."""
    for name, (call, accepted) in _entries(dev, bits).items():
        lo, hi = (0, bits - 2) if accepted is None or accepted[0] == 0 else (1, 63)
        for m in {-1, bits - 1, bits, lo - 1, hi + 1, 64, 200}:
            if not lo <= m <= hi:
                assert call(m) == -3, (name, m)
        if accepted is not None:
            for m in accepted:
                assert call(m) == 0, (name, m)
    _sync(dev)


def test_protocol_entry_points_raise_outside_the_range():
    from moose_amd.protocols import replicated as rep

    sess = StackedSession("cpu", seed=1)
    for bits in (64, 128):
        d = _t(_case(bits, 1, 5)[1])
        x = rep.RepTensor(PLC, bits, "arith", PV(PLC, R.RT(d, bits)),
                          PV(PLC, R.RT(torch.roll(d, -1, 0).contiguous(), bits)))
        for m in (-1, bits - 1, bits):
            for f in (lambda: rep.trunc_pr(sess, x, m), lambda: rep.mul_trunc(sess, x, x, m),
                      lambda: rep.dot_trunc(sess, x, x, m),
                      lambda: rep.mul_public_trunc(sess, x, None, m),
                      lambda: rep.mul_trunc_many(sess, [(x, x, 1, None), (x, x, m, None)]),
                      lambda: rep.mul_add_trunc(sess, x, x, x, m),
                      lambda: rep.dwconv_trunc(sess, x, x, m, {}),
                      lambda: rep.pwl_trunc(sess, x, [0], [1], [0], 1, m),
                      lambda: rep.tail_job(sess, PLC, bits, m, NONCES7, x.s0, None),
                      lambda: rep.StackedTail(sess, PLC, bits, x.s0, m, NONCES7)):
                with pytest.raises(ValueError, match="outside 0"):
                    f()
        assert rep.trunc_pr(sess, x, 0) is x
        y = rep.trunc_pr(sess, x, bits - 2)
        assert tuple(y.s0.v.shape) == tuple(d.shape[:2])
