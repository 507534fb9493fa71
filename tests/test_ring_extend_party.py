"""Per-party ring extension Z_2^64 -> Z_2^128 (csrc/rss_party.hip k_ring_extend_party_r0 / r1,
SPMDSession.party_ring_extend, CyclicSession.party_ring_extend): the kernel pair, its CPU
twin, the stacked fused kernel and the protocol composed from host primitives give the same
share words; the result reveals to the sign extension of the input bit for bit; per-party
threads, the composed one-GPU replay and the cyclic layout run it behind
``replicated.PARTY_RING_EXTEND``."""
import os
import queue
import socket
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import moose_amd as pm
from moose_amd.ir.computation import ReplicatedPlacement
from moose_amd.ops import ring as R
from moose_amd.protocols import replicated as rep
from moose_amd.runtime import keys as K
from moose_amd.runtime.local import LocalMooseRuntime
from moose_amd.utils import telemetry

PLC = ReplicatedPlacement(("a", "b", "c"))
ROLES = ["alice", "bob", "carole"]
M64, M128 = (1 << 64) - 1, (1 << 128) - 1
EDGES = [0, 1, -1, (1 << 62) - 1, -(1 << 62)]
# below, at and across a keystream block's four chunks; around the 64 blocks that ks_chunk
# interleaves over 256 chunks; across a thread block (1024 elements); one 2-D shape
SHAPES = [(1,), (3,), (4,), (5,), (63,), (65,), (257,), (1027,), (7, 13)]
K0, K1, K2 = bytes(range(16)), bytes(range(50, 66)), bytes(range(100, 116))
# component c in role c holds (own k_c, next k_{c+1})
PAIRS = [K0, K1, K1, K2, K2, K0]
NONCES = [1000 + i for i in range(6)]  # r0, r1, R0, M0, z0, z2


def _numel(shape):
    return int(np.prod(shape))


def _mask(n, nonces):
    """r = r0 + r1 (mod 2^64) of every element: the low halves of the 128-bit draws."""
    lo = [R.to_ints(R.RT(R.prf_expand([k], nc, (n,), 128, "cpu").data[0], 128)) for k, nc in
          ((K0, nonces[0]), (K2, nonces[1]))]
    return [(int(a) + int(b)) & M64 for a, b in zip(lo[0], lo[1])]


def _values(n, r, rng):
    """The edge values, then seeded random values in [-2^62, 2^62) -- where the mask allows
    it (r_msb = 1) every other one chosen so that x + 2^62 + r wraps past 2^64."""
    vals = list(EDGES[:n])
    for i in range(len(vals), n):
        if r[i] >> 63 and i % 2:
            xp = int(rng.integers((1 << 64) - r[i], 1 << 63))  # x' + r >= 2^64
        elif r[i] >> 63:
            xp = int(rng.integers(0, (1 << 64) - r[i]))
        else:
            xp = int(rng.integers(0, 1 << 63))
        vals.append(xp - (1 << 62))
    return vals


def _cases(vals, r):
    """(r_msb, c_msb) of every element; (1, 0) is the wrap."""
    out = set()
    for x, ri in zip(vals, r):
        c = (x + (1 << 62) + ri) & M64
        out.add((ri >> 63, c >> 63))
    return out


def _slots(vals, rng):
    """[3, n] share slots of the values over Z_2^64 (x0, x1 uniform)."""
    x0 = [int(v) for v in rng.integers(0, 1 << 64, len(vals), dtype=np.uint64)]
    x1 = [int(v) for v in rng.integers(0, 1 << 64, len(vals), dtype=np.uint64)]
    x2 = [(v - a - b) & M64 for v, a, b in zip(vals, x0, x1)]
    return R.from_ints([x0, x1, x2], 64)


_INPUTS = {}


def _inputs(shape):
    """(values, r, [3, *shape] slots as an int64 tensor) of one case: computed once, shared
    by the tests, never written."""
    if shape not in _INPUTS:
        n = _numel(shape)
        rng = np.random.default_rng(n)
        r = _mask(n, NONCES)
        vals = _values(n, r, rng)
        _INPUTS[shape] = (vals, r, _slots(vals, rng).data.reshape((3,) + tuple(shape)))
    return _INPUTS[shape]


_KEYS = {}


def _key_ptrs(keys, device):
    """Device key-slot images of ``keys`` and their addresses (the images stay alive)."""
    ck = (tuple(keys), str(device))
    if ck not in _KEYS:
        w = K.slot_words(list(keys))
        _KEYS[ck] = torch.from_numpy(w.view(np.int32).copy()).to(device)
    t = _KEYS[ck]
    return [t[i].data_ptr() for i in range(len(keys))]


def _round0(x, device, comps=(0, 1, 2)):
    """Round 0 on ``device`` for the components ``comps`` (component c in role c) of the
    [3, ...] slots ``x``: party c holds (x_c, x_{c+1})."""
    comps = list(comps)
    s0 = x[comps].contiguous().to(device)
    s1 = torch.roll(x, -1, 0)[comps].contiguous().to(device)
    slots = _key_ptrs([k for c in comps for k in PAIRS[2 * c:2 * c + 2]], device)
    return R.ring_extend_party_r0(R.RT(s0, 64), R.RT(s1, 64), comps, slots, NONCES)


def _route(msg, msg_R, msg_M):
    """Round A by hand: msg P0 <-> P1, the dealer's R1 and M1 P2 -> P1."""
    rmk, rR, rM = torch.zeros_like(msg), torch.zeros_like(msg_R), torch.zeros_like(msg_M)
    rmk[0], rmk[1] = msg[1], msg[0]
    rR[1], rM[1] = msg_R[2], msg_M[2]
    return rmk, rR, rM


def _round1(msg, rmk, rR, rM, out0, out1, device, comps=(0, 1, 2)):
    comps = list(comps)
    slots = _key_ptrs([k for c in comps for k in PAIRS[2 * c:2 * c + 2]], device)
    return R.ring_extend_party_r1(msg, rmk, rR, rM, out0, out1, comps, slots, NONCES)


_HOST = {}


def _host_rounds(shape):
    """Both rounds of the CPU twin, three roles stacked, computed once: (round-0 outputs,
    routed messages, w, out0, out1 with every slot filled)."""
    if shape not in _HOST:
        x = _inputs(shape)[2]
        msg, msg_R, msg_M, out0, out1 = _round0(x, "cpu")
        rmk, rR, rM = _route(msg, msg_R, msg_M)
        o0, o1 = out0.clone(), out1.clone()
        w = _round1(msg, rmk, rR, rM, o0, o1, "cpu")
        z1 = R.binary("add", R.RT(w[0], 128), R.RT(w[1], 128)).data  # round 2
        o1[0], o0[1] = z1, z1
        _HOST[shape] = ((msg, msg_R, msg_M, out0, out1), (rmk, rR, rM), w, o0, o1)
    return _HOST[shape]


def _ints(t, bits):
    return [int(v) for v in np.asarray(R.to_ints(R.RT(t.cpu(), bits)), dtype=object).reshape(-1)]


# -- 1. the CPU twin: a replicated sharing of the sign extension, the fused kernel's words ----
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_cpu_twin_three_roles_stacked(shape):
    vals, r, x = _inputs(shape)
    n = _numel(shape)
    _, _, _, out0, out1 = _host_rounds(shape)
    assert out0.shape == (3,) + tuple(shape) + (2,) and out1.shape == out0.shape
    for p in range(3):  # party p's second slot is party p + 1's first
        assert torch.equal(out1[p], out0[(p + 1) % 3])
    z = [_ints(out0[p], 128) for p in range(3)]
    got = [(z[0][i] + z[1][i] + z[2][i]) & M128 for i in range(n)]
    assert got == [v & M128 for v in vals]  # the sign extension, bit for bit
    if n >= 257:  # every (r_msb, c_msb) case, the wrap (1, 0) among them
        assert _cases(vals, r) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # the oracle: the stacked fused kernel's CPU form with the same two keys and six nonces
    ks = _key_ptrs([K0, K2], "cpu")
    f0, f1 = R.ring_extend3_k(R.RT(x.reshape(3, n), 64), ks[0], ks[1], NONCES,
                              out=R.empty2((3, n), 128, "cpu"))
    assert torch.equal(out0.reshape(3, n, 2), f0.data)
    assert torch.equal(out1.reshape(3, n, 2), f1.data)


def test_entry_points_reject_bad_component_counts():
    from moose_amd.ops import native as nat

    lib = nat.lib()
    for dev in (0, 1):  # checked before the host / device dispatch: nothing is launched
        assert lib.mx_ring_extend_party_r0(dev, 0, 3, *[None] * 11) == 0  # n == 0
        assert lib.mx_ring_extend_party_r1(dev, 0, 3, *[None] * 11) == 0
        for ncomp in (0, 4):
            assert lib.mx_ring_extend_party_r0(dev, 5, ncomp, *[None] * 11) == -3
            assert lib.mx_ring_extend_party_r1(dev, 5, ncomp, *[None] * 11) == -3


# -- 2. per-party threads on the CPU --------------------------------------------------------
NARROW = pm.fixed(8, 23, ring=64)
WIDE = pm.fixed(24, 40, ring=128)


def _programs():
    alice, bob, carole = (pm.host_placement(n) for n in ROLES)
    plc = pm.replicated_placement("rep", players=[alice, bob, carole])
    arg = lambda p: pm.Argument(placement=p, vtype=pm.TensorType(pm.float64))  # noqa: E731

    @pm.computation
    def widen(x: arg(alice)):
        with alice:
            xf = pm.cast(x, dtype=NARROW)
        with plc:
            w = pm.cast(xf, dtype=WIDE)
        with carole:
            return pm.cast(w, dtype=pm.float64)

    def dot(wide):
        @pm.computation
        def f(x: arg(alice), y: arg(bob)):
            with alice:
                xf = pm.cast(x, dtype=NARROW)
            with bob:
                yf = pm.cast(y, dtype=NARROW)
            with plc:
                z = pm.dot(xf, yf)
                if wide:
                    z = pm.cast(z, dtype=WIDE)
            with carole:
                return pm.cast(z, dtype=pm.float64)
        return f

    return {"widen": widen, "dot": dot(False), "dot_widen": dot(True)}


PROGRAMS = _programs()
X = np.random.default_rng(0).uniform(-100, 100, (7, 13))
X[0, :3] = [0.0, -2.0 ** -23, 127.5]
WANT = np.trunc(X * 2.0 ** 23) / 2.0 ** 23  # fixed(8, 23) encoding truncates
_RNG = np.random.default_rng(1)
ARGS = {"widen": {"x": X},
        "dot_widen": {"x": _RNG.uniform(-2, 2, (5, 9)), "y": _RNG.uniform(-2, 2, (9, 3))}}
ARGS["dot"] = ARGS["dot_widen"]


def _span_names(fn):
    """The names of the telemetry spans ``fn`` records."""
    old = telemetry._TRACE_PATH
    telemetry._TRACE_PATH = os.devnull
    try:
        with telemetry._EV_LOCK:
            start = len(telemetry._EVENTS)
        res = fn()
        with telemetry._EV_LOCK:
            names = {e["name"] for e in telemetry._EVENTS[start:]}
    finally:
        telemetry._TRACE_PATH = old
    return res, names


@pytest.mark.parametrize("prog", ["widen", "dot_widen"])
def test_threads_runtime_cpu_equals_composed_and_stacked(prog, monkeypatch):
    devs = {r: "cpu" for r in ROLES}

    def run():
        rt = LocalMooseRuntime(ROLES, device_map=devs, seed=7)
        return rt.evaluate_computation(PROGRAMS[prog], ARGS[prog])["output_0"]

    assert rep.PARTY_RING_EXTEND is True  # the default
    on, names_on = _span_names(run)
    monkeypatch.setattr(rep, "PARTY_RING_EXTEND", False)
    off, names_off = _span_names(run)
    assert "rep.ring_extend" in names_on and "rep.ring_extend" in names_off
    assert "rep.ring_extend_party" in names_on and "rep.ring_extend_party" not in names_off
    stacked = LocalMooseRuntime(ROLES, device="cpu", seed=7).evaluate_computation(
        PROGRAMS[prog], ARGS[prog])["output_0"]
    assert np.array_equal(on, off) and np.array_equal(on, stacked)
    if prog == "widen":
        assert np.array_equal(on, WANT)


def test_threads_runtime_stats_two_rounds_per_widening():
    """The widening adds exactly two rounds at every party, with the real byte counts: round A
    8 + 8 + 16 + 8 bytes per element, round B 2 x 16."""
    devs = {r: "cpu" for r in ROLES}
    stats = {}
    for prog in ("dot", "dot_widen"):
        rt = LocalMooseRuntime(ROLES, device_map=devs, seed=7)
        rt.evaluate_computation(PROGRAMS[prog], ARGS[prog])
        stats[prog] = {i: s.as_dict() for i, s in rt.last_stats_by_identity.items()}
    n = 5 * 3  # elements of the product
    for i in ROLES:
        a, b = stats["dot"][i], stats["dot_widen"][i]
        assert b["rounds"] - a["rounds"] == 2
        assert b["reshare_bytes"] - a["reshare_bytes"] == (40 + 32) * n
    # the dealer's only messages of the program's second half are R1 and M1 (alice's and
    # bob's send totals also move with the ring width of the revealed value)
    sent = lambda s, d: (stats["dot_widen"][s]["bytes"].get(f"{s}->{d}", 0)  # noqa: E731
                         - stats["dot"][s]["bytes"].get(f"{s}->{d}", 0))
    assert sent("carole", "bob") == (16 + 8) * n


# -- 3. cyclic layout: three ranks, each party of a session on another rank -------------------
SEED = 5
CYC_SHAPE = (1027,)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _cyc_values(session):
    """Edge values and seeded values in [-2^62, 2^62) of one session."""
    n = _numel(CYC_SHAPE)
    rng = np.random.default_rng(40 + session)
    vals = EDGES + [int(v) for v in rng.integers(-(1 << 62), 1 << 62, n - len(EDGES))]
    return vals


def _cyc_program(sess, xa):
    """share -> ring_extend -> reveal; the shares of the input and of the widened value."""
    from moose_amd.protocols import replicated as rep

    Xs = rep.share(sess, PLC, xa)
    r0 = sess.stats.rounds
    Y = rep.ring_extend(sess, Xs)
    rounds = sess.stats.rounds - r0
    out = rep.reveal(sess, Y, "c")
    assert Y.bits == 128
    return ([t.v.data.clone() for t in (Xs.s0, Xs.s1, Y.s0, Y.s1)], out.v.data.clone(), rounds)


def _cyc_input(session, device="cpu"):
    from moose_amd.runtime.session import HV

    x = R.from_ints(np.array(_cyc_values(session), dtype=object).reshape(CYC_SHAPE), 64)
    return HV("a", R.RT(R.to_device(x.data, device), 64))


def _cyc_worker(rank, world, port, q, device):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from moose_amd.parallel.cyclic import CyclicSession
    from moose_amd.parallel.cyclic import RingComm

    sess = CyclicSession(RingComm(rank, world, device), {"a": 0, "b": 1, "c": 2}, seed=SEED,
                         device=device)
    assert hasattr(sess, "party_ring_extend")
    ts, out, rounds = _cyc_program(sess, _cyc_input(sess.session_of("a"), device))
    keys = {s: sess.session_keys(PLC, s) for s in range(world)}
    q.put((rank, [t.cpu().numpy() for t in ts], out.cpu().numpy(), sess.session_of("c"), rounds,
           keys, sess.comm.messages))
    dist.barrier()
    dist.destroy_process_group()


def _cyc_reference(keys, session):
    """The same program on a non-fused stacked CPU session with that session's keys."""
    from moose_amd.runtime.session import StackedSession

    s = StackedSession("cpu", seed=1)
    s.fused = False
    base = s.setup(PLC)
    s.keytable._write(base, keys)
    return _cyc_program(s, _cyc_input(session))


def _cyc_run(device):
    world = 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_cyc_worker, args=(r, world, port, q, device)) for r in range(world)]
    for p in ps:
        p.start()
    got = {}
    deadline = time.monotonic() + 300
    while len(got) < world:  # fail fast if a worker died instead of waiting out a timeout
        try:
            item = q.get(timeout=2)
            got[item[0]] = item[1:]
        except queue.Empty:
            dead = [p.exitcode for p in ps if p.exitcode not in (None, 0)]
            if dead or time.monotonic() > deadline:
                for p in ps:
                    p.kill()
                raise AssertionError(f"cyclic workers failed: exit codes {dead}")
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    keys = got[0][4]
    refs = {s: _cyc_reference(keys[s], s) for s in range(world)}
    for g in range(world):
        ts, out, s_c, rounds, _, msgs = got[g]
        assert msgs > 0  # the parties really exchanged messages
        assert rounds == 2  # one widening: two rounds on every rank
        for i, t in enumerate(ts):
            for p in range(3):  # component p of rank g = party p of session g - p
                ref = refs[(g - p) % world][0][i][p].numpy()
                assert np.array_equal(t[p], ref), (g, i, p)
        assert np.array_equal(out, refs[s_c][1].numpy())
        assert _ints(torch.from_numpy(out), 128) == [v & M128 for v in _cyc_values(s_c)]


def test_cyclic_gloo_bitwise_equals_composed_stacked():
    _cyc_run("cpu")


# -- 4. on the device -----------------------------------------------------------------------
def _assert_rounds_equal(h, d, comps=(0, 1, 2)):
    """Every output the two kernels define, per role, device against host.  ``h``/``d``:
    (round-0 outputs, w, out0, out1 after round 1) with rows ordered as ``comps``."""
    (msg, msg_R, msg_M, o0, o1), w, p0, p1 = h
    (dmsg, dmsg_R, dmsg_M, do0, do1), dw, dp0, dp1 = d
    for row, role in enumerate(comps):
        if role in (0, 1):  # the opening share and the reshare message
            assert torch.equal(msg[row], dmsg[row].cpu()), role
            assert torch.equal(w[row], dw[row].cpu()), role
        if role == 0:
            assert torch.equal(p0[row], dp0[row].cpu())  # z0
        if role == 1:
            assert torch.equal(p1[row], dp1[row].cpu())  # z2
        if role == 2:  # the dealer: R1, M1 and its own new shares (z2, z0)
            assert torch.equal(msg_R[row], dmsg_R[row].cpu())
            assert torch.equal(msg_M[row], dmsg_M[row].cpu())
            assert torch.equal(o0[row], do0[row].cpu())
            assert torch.equal(o1[row], do1[row].cpu())


def _device_rounds(x, received, comps=(0, 1, 2)):
    """Both rounds on the GPU for ``comps``, round 1 fed with the host's routed messages."""
    comps = list(comps)
    r0 = _round0(x, "cuda", comps)
    rmk, rR, rM = (t[comps].contiguous().cuda() for t in received)
    o0, o1 = r0[3].clone(), r0[4].clone()
    w = _round1(r0[0], rmk, rR, rM, o0, o1, "cuda", comps)
    torch.cuda.synchronize()
    return r0, w, o0, o1


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_hip_kernels_equal_cpu_twin(shape):
    x = _inputs(shape)[2]
    r0, received, w, _, _ = _host_rounds(shape)
    # the host's round-1 outputs before round 2 filled the remaining slots
    o0, o1 = r0[3].clone(), r0[4].clone()
    assert torch.equal(_round1(r0[0], *received, o0, o1, "cpu")[:2], w[:2])  # P2 writes no w
    h = (r0, w, o0, o1)
    _assert_rounds_equal(h, _device_rounds(x, received))
    for role in range(3):  # one component in each single role
        pick = lambda ts: tuple(t[role:role + 1] for t in ts)  # noqa: E731
        hr = (pick(r0), w[role:role + 1], o0[role:role + 1], o1[role:role + 1])
        _assert_rounds_equal(hr, _device_rounds(x, received, [role]), [role])


@pytest.mark.gpu
def test_hip_kernels_equal_cpu_twin_past_the_grid_cap():
    """n = 2^21 + 5: the launch grid is capped at 2048 blocks per component (256 threads, 4
    elements each), so this is the first size at which the grid-stride loop iterates."""
    n = (1 << 21) + 5
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-(1 << 63), (1 << 63) - 1, (3, n), dtype=torch.int64, generator=g)
    r0 = _round0(x, "cpu")
    received = _route(*r0[:3])
    o0, o1 = r0[3].clone(), r0[4].clone()
    w = _round1(r0[0], *received, o0, o1, "cpu")
    _assert_rounds_equal((r0, w, o0, o1), _device_rounds(x, received))


@pytest.mark.gpu
def test_threads_runtime_gpu_replay_uses_the_party_kernels(monkeypatch):
    """Parties as threads on cuda:0, seeded: the composed hipGraph replays equal the eager
    evaluation and the composed-protocol path bitwise, with fewer graph nodes than that
    path (the parent's) and the round kernels party-batched."""
    devs = {r: "cuda:0" for r in ROLES}
    nodes = {}
    outs = {}
    for on in (True, False):
        monkeypatch.setattr(rep, "PARTY_RING_EXTEND", on)
        eager = LocalMooseRuntime(ROLES, device_map=devs, seed=11, use_graphs=False)
        want = eager.evaluate_computation(PROGRAMS["widen"], ARGS["widen"])["output_0"]
        rt = LocalMooseRuntime(ROLES, device_map=devs, seed=11, use_graphs=True)
        for _ in range(4):
            got = rt.evaluate_computation(PROGRAMS["widen"], ARGS["widen"])["output_0"]
            assert np.array_equal(got, want)
        (_, tapes), = rt._party_tapes.values()
        assert tapes is not False and tapes.tapes[0].replays == 2
        nodes[on] = dict(tapes.graph_nodes)
        outs[on] = want
    print("graph nodes, party kernels:", nodes[True], "composed:", nodes[False])
    assert np.array_equal(outs[True], outs[False]) and np.array_equal(outs[True], WANT)
    assert nodes[True]["nodes"] < nodes[False]["nodes"]
    assert nodes[True]["party_batched"] > 0


@pytest.mark.gpu
def test_cyclic_on_gpu_bitwise_equals_composed_stacked():
    """Three party processes sharing the one test GPU (payloads staged through gloo)."""
    _cyc_run("cuda:0")
