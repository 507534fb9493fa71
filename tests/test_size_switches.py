"""The host launchers that pick another kernel by element count, pinned on both sides of
every switch: a latency form below a threshold, a throughput form above it, and capped grids
whose loops take a second trip above a third size (docs/ARCHITECTURE.md, "Size switches").

Every device result is compared bitwise with the CPU twin on identical inputs and key slots,
and -- where a launcher's result has a meaning that needs no key -- with an integer model
written here on numpy ``uint64`` words (pairs of them for Z_2^128) or Python integers:

* the three roles run on consistent replicated shares (party ``p`` holds components ``p`` and
  ``p + 1``), with the real messages between them, so the keystream cancels across the
  parties and what is left is the plain function of the reconstructed values;
* a bug shared by a kernel and its twin (a dropped argument, a wrong chunk walk) fails the
  model on either device, so the model tests carry no ``gpu`` mark and pin the twins too.

The CPU runs are computed once per case and shared between the model tests and the device
tests."""
import functools

import numpy as np
import pytest
import torch

import moose_amd as pm
from moose_amd.ir.computation import ReplicatedPlacement
from moose_amd.ops import native as nat
from moose_amd.ops import ring as R
from moose_amd.protocols import replicated as rep
from moose_amd.runtime.keys import KeyTable
from moose_amd.runtime.local import LocalMooseRuntime
from moose_amd.runtime.session import HV, StackedSession

GPU = pytest.param("cuda", marks=pytest.mark.gpu)
DEVICES = ["cpu", GPU]
KEYS = [bytes(range(16)), bytes(range(16, 32)), bytes(range(32, 48))]
U = np.uint64


# ---------------------------------------------------------------------------
# inputs, key slots and the integer model's words
# ---------------------------------------------------------------------------
def _rand(shape, bits, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-(2**63), 2**63 - 1, tuple(shape) + ((2,) if bits == 128 else ()),
                         generator=g, dtype=torch.int64)


def _slots(dev):
    """Three keys in slots 0..2; party r reads (k_r, k_{r+1})."""
    kt = KeyTable(dev, capacity=4)
    kt._write(0, KEYS)
    return kt, [[kt.ptr(r), kt.ptr((r + 1) % 3)] for r in range(3)]


def _sync(dev):
    if dev != "cpu":
        torch.cuda.synchronize()


def _rt(t, bits, dev):
    return R.RT(t.to(dev), bits)


def _w(t, bits):
    """Ring data (int64, a trailing pair for Z_2^128) -> (lo, hi) uint64 words; hi is None
    for Z_2^64."""
    a = t.detach().cpu().contiguous().numpy().view(U)
    if bits == 128:
        return a[..., 0].copy(), a[..., 1].copy()
    return a.copy(), None


def _map2(f, a, b):
    return f(a[0], b[0]), None if a[1] is None else f(a[1], b[1])


def _xor(a, b):
    return _map2(np.bitwise_xor, a, b)


def _and(a, b):
    return _map2(np.bitwise_and, a, b)


def _xor3(ws):
    return _xor(_xor(ws[0], ws[1]), ws[2])


def _shl(a, d):
    assert 0 < d < 64
    lo = a[0] << U(d)
    if a[1] is None:
        return lo, None
    return lo, (a[1] << U(d)) | (a[0] >> U(64 - d))


def _add(a, b):
    lo = a[0] + b[0]
    if a[1] is None:
        return lo, None
    return lo, a[1] + b[1] + (lo < a[0]).astype(U)


def _bit(a, q):
    """Bit q as a ring element (0 / 1)."""
    w = a[0] if q < 64 else a[1]
    return (w >> U(q % 64)) & U(1), None if a[1] is None else np.zeros_like(a[0])


def _rows(a, lo, hi):
    return a[0][lo:hi], None if a[1] is None else a[1][lo:hi]


def _flat(a):
    return a[0].reshape(-1), None if a[1] is None else a[1].reshape(-1)


def _weq(a, b, what):
    assert np.array_equal(a[0], b[0]), what
    if a[1] is not None:
        assert np.array_equal(a[1], b[1]), what


def _teq(a, b, what):
    if a is None or b is None:
        assert a is None and b is None, what
        return
    assert torch.equal(a.cpu(), b.cpu()), what


def _all_eq(cpu, dev, what):
    assert len(cpu) == len(dev)
    for k, (a, b) in enumerate(zip(cpu, dev)):
        _teq(a, b, f"{what}: tensor {k}")


# ---------------------------------------------------------------------------
# 1. Kogge-Stone level: mx_ks_cross1_s / mx_ks_cross1x_s
#    latency form while ceil((both ? 2n : n) / P) <= 16384 chunks (P = 1 for u128, 2 for u64)
# ---------------------------------------------------------------------------
KS_CASES = [(128, False, 16384), (128, False, 16385), (128, True, 8192), (128, True, 8193),
            (64, False, 32768), (64, False, 32769), (64, True, 16384), (64, True, 16385),
            (128, False, 70001), (128, True, 70001), (64, False, 70001), (64, True, 70001)]


def _ks_components(bits, n):
    """g, t, pk as three boolean share components each."""
    return {k: [_rand((n,), bits, s + c) for c in range(3)]
            for k, s in (("g", 110), ("t", 120), ("pk", 130))}


def _ks_level_run(dev, bits, both, n, d):
    """The three roles' plain and xor-folding level on consistent shares: per role
    [z, zx, go0, go1]."""
    comp = _ks_components(bits, n)
    kt, slots = _slots(dev)
    out = []
    for r in range(3):
        q = (r + 1) % 3
        g0, g1, t0, t1, p0, p1 = (_rt(comp[k][c], bits, dev) for k, c in
                                  (("g", r), ("g", q), ("t", r), ("t", q), ("pk", r), ("pk", q)))
        z = R.ks_cross1_s(g0, g1, p0, p1, d, both, slots[r], 23)
        zx, (go0, go1) = R.ks_cross1x_s(g0, g1, t0, t1, p0, p1, d, both, slots[r], 29)
        _sync(dev)
        out.append([x.data.cpu() for x in (z, zx, go0, go1)])
    del kt
    return out


@functools.lru_cache(maxsize=None)
def _ks_level_cpu(bits, both, n, d):
    return _ks_level_run("cpu", bits, both, n, d)


def _ks_level_model(out, bits, both, n, d):
    comp = _ks_components(bits, n)
    G, T, P = (_xor3([_w(c, bits) for c in comp[k]]) for k in ("g", "t", "pk"))
    for r in range(3):  # go == g ^ t exactly, on both components
        q = (r + 1) % 3
        _weq(_w(out[r][2], bits), _xor(_w(comp["g"][r], bits), _w(comp["t"][r], bits)), f"go0 P{r}")
        _weq(_w(out[r][3], bits), _xor(_w(comp["g"][q], bits), _w(comp["t"][q], bits)), f"go1 P{r}")
    for k, Gk, what in ((0, G, "ks_cross1_s"), (1, _xor(G, T), "ks_cross1x_s")):
        Z = _xor3([_flat(_w(out[r][k], bits)) for r in range(3)])
        assert Z[0].shape == ((2 * n,) if both else (n,))
        _weq(_rows(Z, 0, n), _and(P, _shl(Gk, d)), f"{what}: t = pk & (g << {d})")
        if both:
            _weq(_rows(Z, n, 2 * n), _and(P, _shl(P, d)), f"{what}: pk' = pk & (pk << {d})")


@pytest.mark.parametrize("d", [1, 32])
@pytest.mark.parametrize("bits,both,n", KS_CASES)
def test_ks_level_twin_matches_integer_model(bits, both, n, d):
    """The host twins of ks_cross1_s / ks_cross1x_s at the switch sizes: the XOR of the three
    parties' z is pk & ((g ^ t) << d) (and pk & (pk << d) with both ANDs), go = g ^ t."""
    _ks_level_model(_ks_level_cpu(bits, both, n, d), bits, both, n, d)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 32])
@pytest.mark.parametrize("bits,both,n", KS_CASES)
def test_ks_level_both_sides_of_latency_switch(bits, both, n, d):
    """k_ks_cross1_lat at the last latency size, k_ks_cross1 at the first throughput size and
    well above it: z, go0, go1 equal the host twin's, and the device's own outputs satisfy the
    key-free model (a level that drops the fold of g ^ t fails it)."""
    dev = _ks_level_run("cuda", bits, both, n, d)
    for r, (a, b) in enumerate(zip(_ks_level_cpu(bits, both, n, d), dev)):
        _all_eq(a, b, f"ks level P{r}")
    _ks_level_model(dev, bits, both, n, d)


# ---------------------------------------------------------------------------
# 2. The end-to-end case: three parties as threads on one device, no graph replay
# ---------------------------------------------------------------------------
ROLES = ["alice", "bob", "carole"]
ALICE, BOB, CAROLE = (pm.host_placement(n) for n in ROLES)
REP = pm.replicated_placement("rep", players=[ALICE, BOB, CAROLE])
FX = pm.fixed(24, 40)
BIG = 2.0 ** 24 - 2.0 ** -29  # the largest float64 below 2^24: 2^64 - 2^11 when encoded
TINY = 2.0 ** -40


def _program(op):
    @pm.computation
    def prog(x: pm.Argument(placement=ALICE, vtype=pm.TensorType(pm.float64))):
        with ALICE:
            xf = pm.cast(x, dtype=FX)
        with REP:
            y = pm.relu(xf) if op == "relu" else pm.sort(xf)
        with CAROLE:
            return pm.cast(y, dtype=pm.float64)

    return prog


def _e2e_input(shape):
    """On the 2^-40 grid (the decoded inputs are the inputs): negatives, zeros, and the
    largest and smallest encodable magnitudes of either sign, at the first and last
    positions and inside."""
    rng = np.random.default_rng(shape[0])
    x = np.round(rng.uniform(-100, 100, shape) * 2.0 ** 40) / 2.0 ** 40
    edges = [BIG, -BIG, 0.0, TINY, -TINY, -0.0, 1.0, -1.0]
    flat = x.reshape(-1)
    flat[:len(edges)] = edges
    flat[-len(edges):] = edges[::-1]
    mid = flat.size // 2 - 3
    flat[mid:mid + len(edges)] = edges
    return x


def _threads(device, op, shape):
    rt = LocalMooseRuntime(ROLES, device_map={r: device for r in ROLES}, seed=7,
                           use_graphs=False, fixedpoint_ring=128)
    out = rt.evaluate_computation(_program(op), {"x": _e2e_input(shape)})
    return np.asarray(list(out.values())[0])


@functools.lru_cache(maxsize=None)
def _relu_cpu(shape):
    return _threads("cpu", "relu", shape)


@pytest.mark.parametrize("shape", [(16, 1024), (64, 1024)])
def test_relu_of_party_threads_on_the_host_is_exact(shape):
    """A ReLU multiplies by a flag and truncates nothing: exactly maximum(x, 0)."""
    got = _relu_cpu(shape)
    assert got.shape == shape
    assert np.array_equal(got, np.maximum(_e2e_input(shape), 0))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(16, 1024), (64, 1024)])
def test_relu_of_party_threads_on_one_gpu_without_replay(shape):
    """The per-party sign extraction of 16,384 and of 65,536 elements, eager (no graph
    replay), parties as threads on one GPU: bit for bit the CPU threads' result and exactly
    maximum(x, 0) of the decoded inputs."""
    got = _threads("cuda:0", "relu", shape)
    want = np.maximum(_e2e_input(shape), 0)
    bad = int((got != want).sum())
    print(f"relu {shape}: {bad} wrong entries of {want.size}")
    assert np.array_equal(got, _relu_cpu(shape))
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_sort_of_party_threads_on_one_gpu_without_replay():
    """pm.sort of [64, 1024] (55 compare-exchange stages, each a sign extraction of 32,768
    differences), eager with the parties as threads on one GPU: numpy.sort exactly."""
    shape = (64, 1024)
    got = _threads("cuda:0", "sort", shape)
    want = np.sort(_e2e_input(shape), axis=-1)
    print(f"sort {shape}: {int((got != want).sum())} wrong entries of {want.size}")
    assert np.array_equal(got, want)


# ---------------------------------------------------------------------------
# 3. Per-party bit front and B2A (csrc/rss_bits_party.hip)
#    grid_of caps at 2048 blocks of 64 chunks; B2A takes the throughput form at >= 2048 chunks
# ---------------------------------------------------------------------------
FRONT_N = {128: 131072 + 65, 64: 262144 + 131}  # both past 2048 blocks x 64 chunks


def _front_components(bits, n):
    return [_rand((n,), bits, 210 + c) for c in range(3)]


def _front_run(dev, bits, n):
    """bits_front for the three roles on one arithmetic sharing, P1 after P0's message:
    per role [msg, z, p0, p1]."""
    x = [t.to(dev) for t in _front_components(bits, n)]
    kt, slots = _slots(dev)
    res = {}
    for r in (0, 2, 1):
        a1 = res[0][0] if r == 1 else None
        res[r] = R.bits_front(r, x[r], x[(r + 1) % 3], a1, bits, slots[r], 31, 32)
    _sync(dev)
    del kt
    return [[None if t is None else t.cpu() for t in res[r]] for r in range(3)]


@functools.lru_cache(maxsize=None)
def _front_cpu(bits):
    return _front_run("cpu", bits, FRONT_N[bits])


def _front_model(out, bits, n):
    """p is a sharing of y ^ x2 and z one of y & x2, y = x0 + x1; P_r's second component is
    P_{r+1}'s first."""
    x = [_w(t, bits) for t in _front_components(bits, n)]
    y = _add(x[0], x[1])
    _weq(_xor3([_w(out[r][2], bits) for r in range(3)]), _xor(y, x[2]), "p = a ^ b")
    _weq(_xor3([_w(out[r][1], bits) for r in range(3)]), _and(y, x[2]), "g = a & b")
    for r in range(3):
        _teq(out[r][3], out[(r + 1) % 3][2], f"p1 of P{r}")
    _teq(out[0][0], out[1][2], "P0's message is P1's first component")


@pytest.mark.parametrize("bits", [64, 128])
def test_bits_front_twin_matches_integer_model(bits):
    _front_model(_front_cpu(bits), bits, FRONT_N[bits])


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [64, 128])
def test_bits_front_past_the_grid_cap(bits):
    """k_front with more chunk groups than its 2048 blocks (some blocks take a second trip),
    every role: GPU == CPU, and the device's outputs reconstruct p and g."""
    dev = _front_run("cuda", bits, FRONT_N[bits])
    for r, (a, b) in enumerate(zip(_front_cpu(bits), dev)):
        _all_eq(a, b, f"front P{r}")
    _front_model(dev, bits, FRONT_N[bits])


def _plane_of(row, start, count, xbit, blocks):
    """bits_party.h plane_of, from its description: (plane, xor plane or -1, block, NOT)."""
    nb, sbit = blocks & 0xff, blocks >> 8
    tail = 0 if xbit < 0 else (nb - 1 if nb in (2, 4) else nb)
    if row < count - tail:
        return start + row, xbit, 0, 0
    k = row - (count - tail)
    q = sbit if sbit > 0 else xbit
    if nb == 3:  # NOT sign(z - T), sign(z + T), sign(z)
        return q, -1, (1, 2, 0)[k], int(k == 0)
    if nb == 2:  # sign(x)
        return q, -1, 1, 0
    if nb == 4:  # NOT sign(x - T'), sign(x + T'), sign(x)
        return q, -1, k + 1, int(k == 0)
    return q, -1, 0, 0


def _tail(xbit, blocks):
    nb = blocks & 0xff
    return 0 if xbit < 0 else (nb - 1 if nb in (2, 4) else nb)


def _b2a_components(bits, S, blocks):
    n = S * (blocks & 0xff)
    return {k: [_rand((n,), bits, s + c) for c in range(3)]
            for k, s in (("s", 310), ("g", 320), ("t", 330))}


def _b2a_run(dev, bits, S, count, xbit, blocks, with_g, start=5):
    """Phases 0 / 1 / 2 of the three roles on one boolean sharing of the adder's state, with
    the real messages (P0's A1 to P1, every z to the previous party): per role
    [msg, z, base0, base1, out0, out1]."""
    comp = _b2a_components(bits, S, blocks)
    kt, slots = _slots(dev)
    st = {}
    for r in (0, 2, 1):
        q = (r + 1) % 3
        src = [comp[k][c].to(dev) for k in ("s", "g", "t") for c in (r, q)]
        if not with_g:
            src[2:] = [None] * 4
        st[r] = R.bits_b2a(0 if r != 1 else 1, r, src, start, count, bits, slots[r], 33, 34,
                           arecv=st[0][0] if r == 1 else None, xbit=xbit, blocks=blocks)
    outs = {r: R.bits_b2a(2, r, None, start, count, bits, slots[r], 33, 34,
                          arecv=st[(r + 1) % 3][1], state=st[r], xbit=xbit, blocks=blocks)
            for r in range(3)}
    _sync(dev)
    del kt
    return [[None if t is None else t.cpu() for t in list(st[r]) + list(outs[r])]
            for r in range(3)]


@functools.lru_cache(maxsize=None)
def _b2a_cpu(bits, S, count, xbit, blocks, with_g):
    return _b2a_run("cpu", bits, S, count, xbit, blocks, with_g)


def _b2a_model(out, bits, S, count, xbit, blocks, with_g, start=5):
    """The three parties' outputs are an arithmetic sharing of the bit plane_of names: the
    plane of the reconstructed sum word, XORed with plane xbit, complemented on NOT rows."""
    comp = _b2a_components(bits, S, blocks)
    W = _xor3([_w(c, bits) for c in comp["s"]])
    if with_g:  # raw adder state: sum = p ^ ((g ^ t) << 1)
        GT = _xor(_xor3([_w(c, bits) for c in comp["g"]]), _xor3([_w(c, bits) for c in comp["t"]]))
        W = _xor(W, _shl(GT, 1))
    total = _add(_add(_w(out[0][4], bits), _w(out[1][4], bits)), _w(out[2][4], bits))
    assert total[0].shape == (count, S)
    for row in range(count):
        q, xq, blk, neg = _plane_of(row, start, count, xbit, blocks)
        Wb = _rows(W, blk * S, (blk + 1) * S)
        want = _bit(Wb, q)
        if xq >= 0:
            want = _xor(want, _bit(Wb, xq))
        if neg:
            want = (want[0] ^ U(1), want[1])
        got = (total[0][row], None if total[1] is None else total[1][row])
        _weq(got, want, f"row {row}: plane {q} xor {xq} block {blk} not {neg}")
    for r in range(3):
        _teq(out[r][5], out[(r + 1) % 3][4], f"out1 of P{r}")


# (S, count) by width: 2047 and 2048 keystream chunks (u64: two elements per chunk, the
# second an odd element count), and past the latency form's grid cap of 2048 x 64 chunks
B2A_SWITCH = {128: [(89, 23), (128, 16)], 64: [(178, 23), (315, 13)]}
B2A_CAP = {128: (43713, 3), 64: (87425, 3)}
SIGN_LAYOUTS = [(2, 37, 3), (4, 37, 3), (2, 700, 8), (4, 700, 8)]  # (nb, S, planes)


def _b2a_cases():
    cases = []
    for bits in (64, 128):
        for S, count in B2A_SWITCH[bits]:
            cases.append((bits, S, count, -1, 1, True, False))
            cases.append((bits, S, count, -1, 1, False, False))
        S, count = B2A_CAP[bits]
        cases.append((bits, S, count, -1, 1, True, False))  # the throughput form
        cases.append((bits, S, count, -1, 1, True, True))  # the latency form, forced
        for nb, S, planes in SIGN_LAYOUTS:
            blocks = nb | ((bits - 1) << 8)
            cases.append((bits, S, planes + _tail(60, blocks), 60, blocks, True, False))
    return cases


def _b2a_id(c):
    bits, S, count, xbit, blocks, with_g, lat = c
    return (f"u{bits}-S{S}x{count}-nb{blocks & 0xff}-{'raw' if with_g else 'sums'}"
            f"{'-lat' if lat else ''}")


B2A_CASES = _b2a_cases()


def test_b2a_switch_sizes_are_the_chunk_counts_they_claim():
    for bits in (64, 128):
        per = 2 if bits == 64 else 1
        chunks = [(S * c + per - 1) // per for S, c in B2A_SWITCH[bits]]
        assert chunks == [2047, 2048]
        S, c = B2A_CAP[bits]
        assert (S * c + per - 1) // per > 2048 * 64


@pytest.mark.parametrize("case", [c for c in B2A_CASES if not c[6]], ids=_b2a_id)
def test_bits_b2a_twin_matches_integer_model(case):
    bits, S, count, xbit, blocks, with_g, _lat = case
    _b2a_model(_b2a_cpu(bits, S, count, xbit, blocks, with_g), bits, S, count, xbit, blocks,
               with_g)


@pytest.mark.gpu
@pytest.mark.parametrize("case", B2A_CASES, ids=_b2a_id)
def test_bits_b2a_both_sides_of_throughput_switch(case, monkeypatch):
    """k_b2a below 2048 chunks, k_b2a_tp from there, both past 2048 x 64 chunks (the latency
    form with MOOSEX_B2A_TP set, whose blocks then take a second trip), and the block
    layouts nb = 2 and nb = 4 with the ring's top bit as the sign plane: every role and phase
    GPU == CPU, and the device's outputs reconstruct the bits plane_of names."""
    bits, S, count, xbit, blocks, with_g, lat = case
    if lat:
        monkeypatch.setenv("MOOSEX_B2A_TP", "0")
    dev = _b2a_run("cuda", bits, S, count, xbit, blocks, with_g)
    for r, (a, b) in enumerate(zip(_b2a_cpu(bits, S, count, xbit, blocks, with_g), dev)):
        _all_eq(a, b, f"b2a P{r}")
    _b2a_model(dev, bits, S, count, xbit, blocks, with_g)


# ---------------------------------------------------------------------------
# 4. Stacked and shared launchers of ring_hip.hip with a switch at 65,536
# ---------------------------------------------------------------------------
def _xor_share3(v, bits, seed):
    """[3, n] boolean share slots of v and the same rolled by one party."""
    c0, c1 = _rand(v.shape[:1], bits, seed), _rand(v.shape[:1], bits, seed + 1)
    s0 = torch.stack([c0, c1, v ^ c0 ^ c1])
    return s0, torch.roll(s0, -1, dims=0)


def _adder_inputs(bits, n):
    a, b = _rand((n,), bits, 410), _rand((n,), bits, 411)
    if bits == 128:  # carries that cross the limb boundary and run the whole word
        a[0], b[0] = torch.tensor([-1, -1]), torch.tensor([1, 0])
        a[-1], b[-1] = torch.tensor([-1, 0]), torch.tensor([1, 0])
    else:
        a[0], b[0] = -1, 1
        a[-1], b[-1] = 2**63 - 1, 1
    return a, b


def _adder_run(dev, bits, n, nlev, sum_out):
    a, b = _adder_inputs(bits, n)
    g0, g1 = _xor_share3(a & b, bits, 420)
    p0, p1 = _xor_share3(a ^ b, bits, 430)
    kt = KeyTable(dev, capacity=4)
    kt._write(0, KEYS)
    nonces = [500 + 3 * i for i in range(nlev)]
    args = [_rt(t, bits, dev) for t in (g0, g1, p0, p1)]
    if dev == "cpu" and sum_out:  # the host has the carries only: the sum is p ^ (g << 1)
        G = R.ks_adder3_k(*args, kt.ptr(0), nonces)
        o = [R.binary("xor", p, g.shl(1)) for p, g in zip(args[2:], G)]
    else:
        o = R.ks_adder3_k(*args, kt.ptr(0), nonces, sum_out=sum_out)
    _sync(dev)
    del kt
    return [t.data.cpu() for t in o]


@functools.lru_cache(maxsize=None)
def _adder_cpu(bits, n, nlev, sum_out):
    return _adder_run("cpu", bits, n, nlev, sum_out)


def _adder_model(out, bits, n, nlev, sum_out):
    """The reconstructed sum is a + b; a chain of nlev levels resolves carries over 2^nlev
    bits, so with fewer levels than log2(bits) the low 2^nlev bits are pinned."""
    a, b = _adder_inputs(bits, n)
    o0 = _w(out[0], bits)
    got = _xor3([(o0[0][r], None if o0[1] is None else o0[1][r]) for r in range(3)])
    if not sum_out:  # the carries: sum = p ^ (g << 1)
        got = _xor(_w(a ^ b, bits), _shl(got, 1))
    want = _add(_w(a, bits), _w(b, bits))
    if (1 << nlev) >= bits:
        _weq(got, want, "a + b")
    else:
        assert nlev == 6 and bits == 128
        assert np.array_equal(got[0], want[0]), "a + b, low 64 bits"
    _teq(out[1], torch.roll(out[0], -1, dims=0), "s1 is s0 rolled by one party")


ADDER_CASES = [(bits, n, nlev, sum_out) for bits, nlev in ((64, 6), (128, 6), (128, 7))
               for n in (65536, 65537) for sum_out in (False, True)]


@pytest.mark.parametrize("bits,n,nlev,sum_out", ADDER_CASES)
def test_ks_adder3_twin_is_integer_addition(bits, n, nlev, sum_out):
    _adder_model(_adder_cpu(bits, n, nlev, sum_out), bits, n, nlev, sum_out)


@pytest.mark.gpu
@pytest.mark.parametrize("bits,n,nlev,sum_out", ADDER_CASES)
def test_ks_adder3_both_sides_of_latency_switch(bits, n, nlev, sum_out):
    """mxh_ks_adder3_sum: k_ks_adder3p up to 65,536 elements per party, k_ks_adder3 above;
    carries and sum, 6 and 7 levels: GPU == CPU, and the reconstruction is a + b."""
    dev = _adder_run("cuda", bits, n, nlev, sum_out)
    _all_eq(_adder_cpu(bits, n, nlev, sum_out), dev, "ks_adder3")
    _adder_model(dev, bits, n, nlev, sum_out)


def _cross_run(dev, bits, kind, n):
    xs = [_rt(_rand((3, n), bits, 440 + i), bits, dev) for i in range(4)]
    kt = KeyTable(dev, capacity=4)
    kt._write(0, KEYS)
    z = R.rss_cross_k(kind, *xs, kt.ptr(0), 3, 77, 3)
    _sync(dev)
    del kt
    return xs, z.data.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["arith", "bool"])
@pytest.mark.parametrize("bits,n", [(128, 65536), (128, 65537), (64, 131072), (64, 131073)])
def test_rss_cross_ring3_both_sides_of_latency_switch(bits, n, kind):
    """launch_rss_cross with the three ring keys: k_rss_cross_ring3_lat up to 65,536 chunks,
    k_rss_cross_ring3 above: GPU == CPU; the zero shares cancel, so the parties' terms
    reconstruct x * y (x & y)."""
    xs, cpu = _cross_run("cpu", bits, kind, n)
    _xs, dev = _cross_run("cuda", bits, kind, n)
    _teq(cpu, dev, "rss_cross_k")
    x0, x1, y0, y1 = (t.data for t in xs)
    if kind == "bool":
        want = (x0 & y0) ^ (x0 & y1) ^ (x1 & y0)
        want = want[0] ^ want[1] ^ want[2]
        _teq(dev[0] ^ dev[1] ^ dev[2], want, "cross terms, keystream cancelled")
    elif bits == 64:  # int64 arithmetic wraps as Z_2^64 does
        want = (x0 * y0 + x0 * y1 + x1 * y0).sum(0)
        _teq(dev.sum(0), want, "cross terms, keystream cancelled")


WSUM_CASES = [(15, (2, 32768)), (16, (2, 32768)), (16, (1, 65537))]


def _wsum_run(dev, bits, k, outer, inner):
    a = _rand((outer, k, inner), bits, 450)
    w = [((-1) ** j) * ((j * 7919 + 3) << (j * 9 % (bits - 8))) for j in range(k)]
    return a, w, R.weighted_sum(_rt(a, bits, dev), w, nb=1).data.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("k,oi", WSUM_CASES)
def test_weighted_sum_both_sides_of_wide_switch(bits, k, oi):
    """mxh_weighted_sum: k_weighted_sum_wide for k >= 16 and at most 65,536 outputs,
    k_weighted_sum otherwise: GPU == CPU, and 257 sampled outputs (the first, the last and
    index 65,535 among them) equal the Python-integer dot mod 2^bits."""
    outer, inner = oi
    a, w, cpu = _wsum_run("cpu", bits, k, outer, inner)
    _a, _w_, dev = _wsum_run("cuda", bits, k, outer, inner)
    _teq(cpu, dev, "weighted_sum")
    total = outer * inner
    idx = {0, total - 1, 65535}
    idx |= set(range(11, total, 257)[:257 - len(idx)])  # 11 + 257 i: none of the three above
    assert len(idx) == 257
    ai, gi = R.to_ints(R.RT(a, bits)), R.to_ints(R.RT(dev, bits)).reshape(-1)
    for g in idx:
        o, i = divmod(g, inner)
        want = sum(w[j] * int(ai[o, j, i]) for j in range(k)) % (1 << bits)
        assert int(gi[g]) == want, (g, k, bits)


def _sum_axis(a, bits, outer, red, inner):
    """mx_sum_axis itself, for both widths (R.sum reduces Z_2^64 with torch)."""
    out = R.empty((outer, inner), bits, a.device)
    nat.check(nat.lib().mx_sum_axis(nat.dev_of(a), bits // 64, nat.ptr(a), nat.ptr(out.data),
                                    outer, red, inner, nat.stream_of(a)), "sum_axis")
    return out.data


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("red,outer,inner", [(1023, 3, 11), (1024, 3, 11), (8, 1, 65537)])
def test_sum_axis_both_sides_of_wide_switch(bits, red, outer, inner):
    """mxh_sum_axis: k_sum_axis_wide (a block per output) for red >= 1024 and at most 65,536
    outputs, k_sum_axis otherwise: (red, outputs) = (1023, 33), (1024, 33), (8, 65537).
    GPU == CPU and, on sampled outputs, the Python-integer sum.  The pair (1024, 65537) --
    both conditions at their edge at once -- needs about a gigabyte of input and is left
    out."""
    a = _rand((outer, red, inner), bits, 460)
    cpu = _sum_axis(a, bits, outer, red, inner)
    dev = _sum_axis(a.cuda(), bits, outer, red, inner)
    torch.cuda.synchronize()
    _teq(cpu, dev, "sum_axis")
    ai, gi = R.to_ints(R.RT(a, bits)), R.to_ints(R.RT(dev.cpu(), bits))
    for o, i in {(0, 0), (outer - 1, inner - 1), (outer // 2, inner // 2)}:
        assert int(gi[o, i]) == sum(int(v) for v in ai[o, :, i]) % (1 << bits)


def _bitdec_input(bits, n):
    x = _rand((n,), bits, 470)
    edge = [0, 1, -1, 2**63 - 1, -(2**63)]  # low words; the high word follows the seed
    for i, v in enumerate(edge):
        if bits == 128:
            x[i, 0] = v
            x[-1 - i, 1] = v
        else:
            x[i] = v
    return x


def _bitdec_run(dev, bits, n):
    plc = ReplicatedPlacement(("a", "b", "c"))
    s = StackedSession(dev, seed=9)
    X = rep.share(s, plc, HV("b", _rt(_bitdec_input(bits, n), bits, dev)))
    B = rep.bit_decompose(s, X)
    L = rep.less_than_zero_arith(s, X)
    _sync(dev)
    return [t.v.data.cpu() for t in (B.s0, B.s1, L.s0, L.s1)]


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("n", [65536, 65537])
def test_stacked_bit_decompose_both_sides_of_fused_limit(bits, n):
    """k_bitdec3 serves up to 65,536 elements; above, the stacked session composes the
    protocol steps: the shares of rep.bit_decompose and of the sign are bitwise the CPU
    session's on both sides, the packed boolean sharing opens to the input's two's-complement
    bits (the word itself) and the sign to its top bit."""
    cpu, dev = _bitdec_run("cpu", bits, n), _bitdec_run("cuda", bits, n)
    _all_eq(cpu, dev, "bit_decompose / sign")
    x = _w(_bitdec_input(bits, n), bits)
    for out in (cpu, dev):
        b0 = _w(out[0], bits)
        _weq(_xor3([(b0[0][r], None if b0[1] is None else b0[1][r]) for r in range(3)]), x,
             "opened bits")
        l0 = _w(out[2], bits)
        parts = [(l0[0][r], None if l0[1] is None else l0[1][r]) for r in range(3)]
        _weq(_add(_add(parts[0], parts[1]), parts[2]), _bit(x, bits - 1), "opened sign")
        _teq(out[1], torch.roll(out[0], -1, dims=0), "s1 of the bits")
        _teq(out[3], torch.roll(out[2], -1, dims=0), "s1 of the sign")


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [64, 128])
def test_ks_sum2_past_the_elementwise_grid_cap(bits):
    """mxd::grid_for caps at 2048 blocks of 256 threads: k_ks_sum2 over 524,288 + 3 elements
    (some threads take a second trip): GPU == CPU == p ^ ((g ^ t) << 1)."""
    n = 524288 + 3
    xs = [_rand((n,), bits, 480 + i) for i in range(6)]
    cpu = R.ks_sum2(*[_rt(t, bits, "cpu") for t in xs])
    dev = R.ks_sum2(*[_rt(t, bits, "cuda") for t in xs])
    torch.cuda.synchronize()
    for c in range(2):
        _teq(cpu[c].data, dev[c].data, f"ks_sum2 component {c}")
        p, g, t = (_w(xs[c + 2 * i], bits) for i in range(3))
        _weq(_w(dev[c].data, bits), _xor(p, _shl(_xor(g, t), 1)), f"ks_sum2 model {c}")
