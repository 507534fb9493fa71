"""The opened dot tail (mx_mul_trunc3_open; rep.StackedTail / ring.OpenedTail): a fixed-point
dot of a stacked device session that is only revealed runs zero share + reshare + TruncPr +
reveal + decode as one kernel.  It must be bitwise the ordinary tail followed by the reveal's
add + decode (mx_mul_trunc3_kv, mx_addn_decode), on the kernel level (host twin and device,
both rings, every launch form) and through the runtime, with the same SessionStats."""
import functools

import numpy as np
import pytest
import torch

import moose_amd as pm
from moose_amd.ir.computation import ReplicatedPlacement
from moose_amd.ops import native as nat
from moose_amd.ops import ring as R
from moose_amd.protocols import replicated as rep
from moose_amd.runtime.session import PV
from moose_amd.runtime.session import StackedSession

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
PLC = ReplicatedPlacement(("alice", "bob", "carole"))
NMUL, NONCES = 0x1234, (11, 12, 13, 14, 15, 16)
FRAC = 23


def _sizes(bits):
    """Element counts per party: around the 4- (u128) / 8-element (u64) ChaCha chunk, several
    blocks of the latency kernel, the last latency and first throughput size (8192 chunks)
    and a throughput launch of several workgroups."""
    per = 16 // (bits // 8)
    return [1, 3, 4, 5, 255, 1023, 4097, 8192 * per, 8192 * per + 1, 70001]


def _ms(bits):
    """Shifts inside TruncPr's range 1 .. bits - 2 (csrc/moosex.h): mx_mul_trunc3_kv and
    mx_trunc_pr3_k, the other side of the comparison, refuse a larger one."""
    return [1, 23, 63, 40] if bits == 128 else [1, 23, 62]


def _stack(n, bits, seed):
    g = torch.Generator().manual_seed(seed)
    shp = (3, n, 2) if bits == 128 else (3, n)
    return torch.randint(-(2**63), 2**63 - 1, shp, generator=g, dtype=torch.int64)


def _bits_of(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def _two_kernels(sess, z: R.RT, m, j=2):
    """The unfused result: the ordinary tail's shares, then the reveal to party j's fused
    add + decode.  The device runs mx_mul_trunc3_kv; the host composes the same protocol
    steps (mx_rss_mul3_k with the product given, mx_trunc_pr3_k), as its sessions do."""
    slot = sess.key_ptr(PLC, 0)
    if z.data.is_cuda:
        s0, s1 = R.zs_trunc3_k(z, slot, NMUL, m, NONCES)
    else:
        p0, p1 = R.rss_mul3_k("arith", z, None, None, None, slot, NMUL)
        x = rep.RepTensor(PLC, z.bits, "arith", PV(PLC, p0), PV(PLC, p1))
        t0, t1 = sess.fused_trunc_pr(x, m, NONCES)
        s0, s1 = t0.v, t1.v
    j1 = (j + 1) % 3
    return R.decode(R.opened(R.RT(s0.data[j], z.bits), R.RT(s1.data[j], z.bits),
                             R.RT(s1.data[j1], z.bits)), FRAC)


@functools.lru_cache(maxsize=None)
def _host_open(bits, m, n):
    """The host twin's output (float64 bit patterns), computed once per case."""
    sess = StackedSession("cpu", seed=7)
    z = R.RT(_stack(n, bits, n), bits)
    out = R.zs_trunc3_open(z, sess.key_ptr(PLC, 0), NMUL, m, NONCES, FRAC)
    return _bits_of(out)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("bits", [64, 128])
def test_open_kernel_matches_tail_then_addn_decode(dev, bits):
    sess = StackedSession(dev, seed=7)
    slot = sess.key_ptr(PLC, 0)
    for m in _ms(bits):
        for n in _sizes(bits):
            z = R.RT(_stack(n, bits, n).to(dev), bits)
            got = R.zs_trunc3_open(z, slot, NMUL, m, NONCES, FRAC)
            assert got.dtype == torch.float64 and tuple(got.shape) == (n,)
            want = _two_kernels(sess, z, m, j=n % 3)
            assert torch.equal(_bits_of(got), _bits_of(want)), (m, n)
            # host twin and device agree bitwise (the same seeded keys)
            assert torch.equal(_bits_of(got), _host_open(bits, m, n)), (m, n)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("bits", [64, 128])
def test_open_kernel_reads_rows_of_a_larger_stack(dev, bits):
    """A non-contiguous product stack (rows of a larger buffer, each party's slot dense) is
    read in place and gives the same result."""
    sess = StackedSession(dev, seed=7)
    slot = sess.key_ptr(PLC, 0)
    w = 2 if bits == 128 else 1
    for rows, cols in ((3, 5), (41, 100), (70, 1001)):
        big = _stack(2 * rows * cols, bits, rows).to(dev).reshape((3, 2 * rows, cols * w))
        if bits == 128:
            big = big.reshape(3, 2 * rows, cols, 2)
        view = R.RT(big[:, rows // 2:rows // 2 + rows], bits)
        assert not view.data.is_contiguous()
        dense = R.RT(view.data.contiguous(), bits)
        got = R.zs_trunc3_open(view, slot, NMUL, 23, NONCES, FRAC)
        want = R.zs_trunc3_open(dense, slot, NMUL, 23, NONCES, FRAC)
        assert tuple(got.shape) == (rows, cols)
        assert torch.equal(_bits_of(got), _bits_of(want))
        assert torch.equal(_bits_of(got), _bits_of(_two_kernels(sess, dense, 23)))


# -- through the runtime ---------------------------------------------------------------------
alice, bob, carole, dave = (pm.host_placement(n) for n in ("alice", "bob", "carole", "dave"))
replicated = pm.replicated_placement("rep", players=[alice, bob, carole])
FX = pm.fixed(14, 23)
F64 = pm.TensorType(pm.float64)


def _dot_reveal(to=carole):
    @pm.computation
    def comp(x: pm.Argument(placement=alice, vtype=F64),
             y: pm.Argument(placement=bob, vtype=F64)):
        with alice:
            xf = pm.cast(x, dtype=FX)
        with bob:
            yf = pm.cast(y, dtype=FX)
        with replicated:
            z = pm.dot(xf, yf)
        with to:
            out = pm.cast(z, dtype=pm.float64)
        return out

    return comp


def _dot_reveal_reuse():
    @pm.computation
    def comp(x: pm.Argument(placement=alice, vtype=F64),
             y: pm.Argument(placement=bob, vtype=F64)):
        with alice:
            xf = pm.cast(x, dtype=FX)
        with bob:
            yf = pm.cast(y, dtype=FX)
        with replicated:
            z = pm.dot(xf, yf)
        with carole:
            out1 = pm.cast(z, dtype=pm.float64)
        with replicated:
            zz = pm.add(z, z)
        with carole:
            out2 = pm.cast(zz, dtype=pm.float64)
        return out1, out2

    return comp


def _args(shapes):
    (a, b), (_, c) = shapes
    rng = np.random.default_rng(5)
    return {"x": rng.uniform(-1, 1, (a, b)), "y": rng.uniform(-1, 1, (b, c))}


class _Calls:
    """Counts the launches of the kernels in question (the library handle's entry points)."""

    NAMES = ("mx_mul_trunc3_open", "mx_mul_trunc3_kv", "mx_addn_decode")

    def __init__(self, monkeypatch):
        self.n = {k: 0 for k in self.NAMES}
        self.captured = {k: 0 for k in self.NAMES}
        lib = nat.lib()
        for name in self.NAMES:
            monkeypatch.setattr(lib, name, self._wrap(name, getattr(lib, name)), raising=False)

    def _wrap(self, name, fn):
        def call(*a):
            self.n[name] += 1
            if torch.cuda.is_current_stream_capturing():
                self.captured[name] += 1
            return fn(*a)

        return call


def _run(comp, args, ring, monkeypatch, open_on, identities=("alice", "bob", "carole")):
    monkeypatch.setenv("MOOSEX_DOT_OPEN", "1" if open_on else "0")  # read at every dot
    calls = _Calls(monkeypatch)
    rt = pm.LocalMooseRuntime(list(identities), device="cuda:0", seed=21, use_graphs=False,
                              fixedpoint_ring=ring)
    outs = rt.evaluate_computation(comp, args)
    return outs, rt.last_stats.as_dict(), dict(calls.n)


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k]).view(np.int64), np.asarray(b[k]).view(np.int64)), k


def _same_stats(a, b):
    for k in ("rounds", "reshare_bytes", "bytes", "messages"):
        assert a[k] == b[k], k


@pytest.mark.gpu
@pytest.mark.parametrize("ring", [64, 128])
@pytest.mark.parametrize("shapes", [((256, 256), (256, 256)), ((256, 384), (384, 512))])
def test_session_dot_reveal_matches_unfused(ring, shapes, monkeypatch):
    comp, args = _dot_reveal(), _args(shapes)
    on, st_on, n_on = _run(comp, args, ring, monkeypatch, True)
    off, st_off, n_off = _run(comp, args, ring, monkeypatch, False)
    _same(on, off)
    _same_stats(st_on, st_off)
    # one kernel instead of two, not one more
    assert n_on == {"mx_mul_trunc3_open": 1, "mx_mul_trunc3_kv": 0, "mx_addn_decode": 0}
    assert n_off == {"mx_mul_trunc3_open": 0, "mx_mul_trunc3_kv": 1, "mx_addn_decode": 1}
    ref = args["x"] @ args["y"]
    assert np.abs(np.asarray(on["output_0"]) - ref).max() < 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("ring", [64, 128])
def test_value_revealed_and_reused(ring, monkeypatch):
    """The shares are read after the value was opened: the ordinary tail runs then, on the
    same keys and nonces, so both outputs equal the unfused run's."""
    comp, args = _dot_reveal_reuse(), _args(((256, 256), (256, 256)))
    on, st_on, n_on = _run(comp, args, ring, monkeypatch, True)
    off, st_off, _ = _run(comp, args, ring, monkeypatch, False)
    _same(on, off)
    _same_stats(st_on, st_off)
    assert n_on["mx_mul_trunc3_open"] == 1 and n_on["mx_mul_trunc3_kv"] == 1


@pytest.mark.gpu
def test_shares_read_before_the_decode(monkeypatch):
    """Protocol level: reveal, then read the shares, then decode -- the decode falls back to
    the ordinary reveal of the shares that now exist; same bits as opening first."""
    bits, M = 128, 256
    outs = []
    for order in ("open_first", "shares_first"):
        sess = StackedSession("cuda", seed=3)
        x0 = R.RT(_stack(M * M, bits, 1).reshape(3, M, M, 2).to("cuda"), bits)
        y0 = R.RT(_stack(M * M, bits, 2).reshape(3, M, M, 2).to("cuda"), bits)
        roll = lambda t: R.RT(torch.roll(t.data, -1, dims=0).contiguous(), bits)  # noqa: E731
        X = rep.RepTensor(PLC, bits, "arith", PV(PLC, x0), PV(PLC, roll(x0)))
        Y = rep.RepTensor(PLC, bits, "arith", PV(PLC, y0), PV(PLC, roll(y0)))
        z = rep.dot_trunc(sess, X, Y, 23)
        assert isinstance(z, rep.StackedTail) and rep.lazy(z)
        hv = rep.reveal(sess, z, "carole")
        assert isinstance(hv.v, R.OpenedTail)
        if order == "shares_first":
            rep.settle(z)
            assert not rep.lazy(z)
        out = R.decode(hv.v, 23)
        assert z.done == (order == "shares_first")
        s0, s1 = z.s0.v, z.s1.v  # read after the opening: the ordinary tail
        sums = R.decode(R.opened(R.RT(s0.data[2], bits), R.RT(s1.data[2], bits),
                                 R.RT(s1.data[0], bits)), 23)
        assert torch.equal(_bits_of(out), _bits_of(sums))
        outs.append((_bits_of(out), _bits_of(s0.data), _bits_of(s1.data)))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_reveal_to_a_non_member_takes_the_ordinary_path(monkeypatch):
    comp, args = _dot_reveal(to=dave), _args(((256, 256), (256, 256)))
    ids = ("alice", "bob", "carole", "dave")
    on, st_on, n_on = _run(comp, args, 128, monkeypatch, True, ids)
    off, st_off, _ = _run(comp, args, 128, monkeypatch, False, ids)
    _same(on, off)
    _same_stats(st_on, st_off)
    assert n_on["mx_mul_trunc3_open"] == 0 and n_on["mx_mul_trunc3_kv"] == 1


@pytest.mark.gpu
def test_captured_replay_holds_the_opening_kernel(monkeypatch):
    """Under use_graphs=True the capture records the opening kernel and no add + decode;
    every evaluation (eager warm-up, then replays with fresh keys) is within TruncPr's
    error of float64: one unit in the last place of fixed(14, 23) from the probabilistic
    truncation plus the operands' encoding error, 256 * 2 * 2^-24 -- below 1e-4."""
    monkeypatch.setenv("MOOSEX_DOT_OPEN", "1")
    calls = _Calls(monkeypatch)
    comp = _dot_reveal()
    rt = pm.LocalMooseRuntime(["alice", "bob", "carole"], device="cuda:0", use_graphs=True)
    rng = np.random.default_rng(8)
    for i in range(3):
        args = {"x": rng.uniform(-1, 1, (256, 256)), "y": rng.uniform(-1, 1, (256, 256))}
        out = rt.evaluate_computation(comp, args)["output_0"]
        assert np.abs(np.asarray(out) - args["x"] @ args["y"]).max() < 1e-4, i
    plan = next(iter(rt._graphs.plans.values()))
    assert plan.replays == 2
    assert calls.captured == {"mx_mul_trunc3_open": 1, "mx_mul_trunc3_kv": 0,
                              "mx_addn_decode": 0}
