"""The per-party TruncPr and dot-tail round bodies (csrc/party_rounds.h; the kernels of
csrc/rss_party.hip and csrc/rss_jobs.hip and their host twins) are one protocol behind three
ways of finding the operands: dense stacked rows (trunc_party), per-component pointers
(dot_tail) and job rows (jobs).  These tests pin the identities between the entry points that
sharing one body relies on, at the sizes where the keystream walk can go wrong -- one element,
the chunk tail of a u64 pair, either side of the 64-chunk stride between a ChaCha block's
parts, either side of a whole block -- and the device kernels against their host twins for
stacked components in every role rotation and past the launch-grid cap."""
import ctypes

import numpy as np
import pytest
import torch

from moose_amd.ops import native as nat
from moose_amd.ops import ring as R
from moose_amd.runtime import keys as K

M = 23
SIZES = [(128, n) for n in (1, 63, 65, 257)] + [(64, n) for n in (1, 3, 129, 515)]
ROTATIONS = [[0, 1, 2], [1, 2, 0], [2, 0, 1]]
KEYS = [bytes(range(16)), bytes(range(50, 66)), bytes(range(100, 116))]
NONCES = [2000 + i for i in range(7)]  # a, r0, r1, t, m, z0, z2 (trunc_party: without a)
FILL = 0x5A5A5A5A5A5A5A5A  # what an output holds where no role writes it
# Z_2^128: the launch grid is capped at 2048 blocks of 256 threads per component, a thread
# walks one ChaCha block = 4 chunks = 4 elements, so this is where the grid-stride loop of
# the walk takes a second trip
N_PAST_CAP = 4 * 2048 * 256 + 5


def _rand(shape, bits, seed, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(-(1 << 63), (1 << 63) - 1, tuple(shape) + ((2,) if bits == 128 else ()),
                      generator=g, dtype=torch.int64)
    return t.to(device)


def _filled(device):
    """alloc(shape[, dtype]) for the ops' outgoing buffers: prefilled, so a whole-tensor
    comparison also checks which elements a call leaves alone."""
    return lambda shape, dtype=torch.int64: torch.full(tuple(shape), FILL, dtype=torch.int64,
                                                       device=device)


_KEYS = {}


def _slots(roles, device):
    """Key-slot addresses of stacked components: one in role r holds (own k_r, next k_{r+1})."""
    if str(device) not in _KEYS:
        img = K.slot_words(KEYS).view(np.int32).copy()
        _KEYS[str(device)] = torch.from_numpy(img).to(device)
    t = _KEYS[str(device)]
    return [t[k % 3].data_ptr() for r in roles for k in (r, r + 1)]


def _vp(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _dot_r0(cross, rt_on, roles, bits, n, device):
    """mx_dot_tail_r0 with any pattern of null pointers: ``cross[c]`` None = no main part,
    ``rt_on[c]`` False = no dealer part.  Returns per-component lists msg, rt, rm, out0,
    out1, every buffer prefilled."""
    new = _filled(device)
    shp = (n,) + ((2,) if bits == 128 else ())
    msg = [None if x is None else new(shp) for x in cross]
    rt = [new(shp) if on else None for on in rt_on]
    rm = [new((n,)) if on else None for on in rt_on]
    out0, out1 = [new(shp) for _ in roles], [new(shp) for _ in roles]
    nat.check(nat.lib().mx_dot_tail_r0(
        nat.dev_of(out0[0]), bits // 64, n, M, len(roles), R._roles_arr(roles),
        _vp(cross), _vp(msg), _vp(rt), _vp(rm), _vp(out0), _vp(out1),
        R._slots_arr(_slots(roles, device)), R._nonces_arr(NONCES),
        nat.stream_of(out0[0])), "dot_tail_r0")
    return msg, rt, rm, out0, out1


def _dot_r1(msg, rmk, rz, rrt, rrm, roles, bits, n, device):
    new = _filled(device)
    shp = (n,) + ((2,) if bits == 128 else ())
    out0, out1 = [new(shp) for _ in roles], [new(shp) for _ in roles]
    w = R.dot_tail_r1(msg, rmk, rz, rrt, rrm, bits, M, roles, _slots(roles, device), NONCES,
                      out0, out1, n, alloc=new)
    return w, out0, out1


def _eq(a, b):
    """Bitwise equality of two (lists of) tensors / None, on the host."""
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_eq(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    return torch.equal(a.cpu(), b.cpu())


# ---------------------------------------------------------------------------------------
# CPU: the identities between the entry points
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,n", SIZES)
def test_dot_tail_r1_without_z2_is_trunc_party_r1(bits, n):
    """(a) the same messages, roles, slots and nonces: w and the new shares bitwise, and
    neither writes anything for the dealer's component."""
    roles = [0, 1, 2]
    msg, rmk, rrt = (_rand((3, n), bits, s) for s in (1, 2, 3))
    rrm = _rand((3, n), 64, 4)
    new = _filled("cpu")
    o0, o1 = new(msg.shape), new(msg.shape)
    w = R.trunc_party_r1(msg, rmk, rrt, rrm, o0, o1, bits, M, roles, _slots(roles, "cpu"),
                         NONCES[1:], alloc=new)
    rows = lambda t: [t[c] for c in range(3)]  # noqa: E731 - dense rows as components
    dw, d0, d1 = _dot_r1(rows(msg), rows(rmk), [None] * 3, rows(rrt), rows(rrm), roles, bits,
                         n, "cpu")
    assert dw[2] is None and _eq(w[2], new(w[2].shape))
    assert _eq(rows(w)[:2], dw[:2])
    assert _eq(rows(o0), d0) and _eq(rows(o1), d1)
    assert not _eq(o0[0], new(o0[0].shape)) and not _eq(o1[1], new(o1[1].shape))


@pytest.mark.parametrize("roles", ROTATIONS, ids=str)
@pytest.mark.parametrize("bits,n", SIZES)
def test_dot_tail_r0_stacked_equals_single_components(bits, n, roles):
    """(b) three stacked components = three one-component calls."""
    cross = [_rand((n,), bits, 10 + c) for c in range(3)]
    rt_on = [r == 2 for r in roles]
    got = _dot_r0(cross, rt_on, roles, bits, n, "cpu")
    for c in range(3):
        one = _dot_r0([cross[c]], [rt_on[c]], [roles[c]], bits, n, "cpu")
        assert _eq([t[c] for t in got], [t[0] for t in one]), (roles, c)


@pytest.mark.parametrize("bits,n", SIZES)
def test_dot_tail_dealer_then_main_equals_combined(bits, n):
    """(c) the dealer's part alone (no products, the other roles off) and then the main part
    alone write what the combined call writes."""
    roles = [0, 1, 2]
    cross = [_rand((n,), bits, 20 + c) for c in range(3)]
    dealer = [r == 2 for r in roles]
    both = _dot_r0(cross, dealer, roles, bits, n, "cpu")
    only = [r if r == 2 else -1 for r in roles]
    _, rt, rm, out0, out1 = _dot_r0([None] * 3, dealer, only, bits, n, "cpu")
    msg, rt2, rm2, m0, m1 = _dot_r0(cross, [False] * 3, roles, bits, n, "cpu")
    assert _eq(both, (msg, rt, rm, out0, out1))
    untouched = _filled("cpu")(m0[0].shape)
    assert rt2 == [None] * 3 and rm2 == [None] * 3
    assert all(_eq(t, untouched) for t in m0 + m1)  # the main part writes no share


@pytest.mark.parametrize("bits,n", SIZES)
def test_dealer_is_one_protocol_in_trunc_party_dot_tail_and_jobs(bits, n):
    """(d) equal slots and nonces: rt1, rm1 and the dealer's new shares bitwise equal from
    trunc_party_r0, dot_tail_r0 and jobs_r0 with one dense job."""
    slots = _slots([2], "cpu")
    new = _filled("cpu")
    x = _rand((1, n), bits, 30)
    t_rt, t_rm, t_o0, t_o1 = R.trunc_party_r0(R.RT(x, bits), R.RT(x, bits), M, [2], slots,
                                              NONCES[1:])
    _, d_rt, d_rm, d_o0, d_o1 = _dot_r0([x[0]], [True], [2], bits, n, "cpu")
    j_o0, j_o1 = new(x[0].shape), new(x[0].shape)
    job = R.MulJob(1, j_o0, j_o1, a=x[0], sa=n)
    _, j_rt, j_rm = R.jobs_r0([job], n, bits, M, 2, slots, NONCES, like=x, alloc=new)
    for got in ((d_rt[0], d_rm[0], d_o0[0], d_o1[0]), (j_rt, j_rm, j_o0, j_o1)):
        assert _eq(got, (t_rt[0], t_rm[0], t_o0[0], t_o1[0]))


# ---------------------------------------------------------------------------------------
# GPU: the kernels against their host twins
# ---------------------------------------------------------------------------------------
def _dot_rounds(roles, bits, n, device, cross_cpu, recv_cpu):
    """Every output of the three dot-tail rounds for stacked components ``roles``.  Round 0:
    the combined call, one with a null-cross component (the dealer's: its dealer part only)
    and one without msg_rt (no dealer part).  Round 1: the three-term opening and the
    two-term one (rz None), on the given received messages.  Round 2: the sums."""
    to = lambda ts: [None if t is None else t.to(device) for t in ts]  # noqa: E731
    cross = to(cross_cpu)
    dealer = [r == 2 for r in roles]
    out = [_dot_r0(cross, dealer, roles, bits, n, device),
           _dot_r0([None if d else x for x, d in zip(cross, dealer)], dealer, roles, bits, n,
                   device),
           _dot_r0(cross, [False] * 3, roles, bits, n, device)]
    msg = out[0][0]
    rmk, rz, rrt, rrm = (to(t) for t in recv_cpu)
    for z in (rz, [None] * 3):
        out.append(_dot_r1(msg, rmk, z, rrt, rrm, roles, bits, n, device))
    w = out[-1][0]
    sums = [_filled(device)(msg[0].shape) for _ in roles]
    R.dot_tail_r2(w, rmk, sums, bits, roles, n)
    out.append(sums)
    if device != "cpu":
        torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("roles", ROTATIONS, ids=str)
@pytest.mark.parametrize("bits,n", [(128, 257), (64, 515)])
def test_dot_tail_kernels_equal_host_twin_stacked(bits, n, roles):
    cross = [_rand((n,), bits, 40 + c) for c in range(3)]
    recv = [[_rand((n,), bits, 50 + 3 * k + c) for c in range(3)] for k in range(3)]
    recv.append([_rand((n,), 64, 60 + c) for c in range(3)])
    host = _dot_rounds(roles, bits, n, "cpu", cross, recv)
    dev = _dot_rounds(roles, bits, n, "cuda", cross, recv)
    for k, (h, d) in enumerate(zip(host, dev)):
        assert _eq(h, d), (roles, k)


@pytest.mark.gpu
def test_trunc_party_kernels_equal_host_twin_past_the_grid_cap():
    bits, n, roles = 128, N_PAST_CAP, [0, 1, 2]
    s0, s1, rmk, rrt = (_rand((3, n), bits, 70 + k) for k in range(4))
    rrm = _rand((3, n), 64, 74)
    res = {}
    for device in ("cpu", "cuda"):
        new = _filled(device)
        r0 = R.trunc_party_r0(R.RT(s0.to(device), bits), R.RT(s1.to(device), bits), M, roles,
                              _slots(roles, device), NONCES[1:], alloc=new)
        msg, msg_rm, out0, out1 = r0  # msg: m0, m1 and the dealer's rt1; msg_rm: its rm1
        o0, o1 = new(msg.shape), new(msg.shape)
        w = R.trunc_party_r1(msg, rmk.to(device), rrt.to(device), rrm.to(device), o0, o1,
                             bits, M, roles, _slots(roles, device), NONCES[1:], alloc=new)
        # round 0 defines the new shares of the dealer's row only
        res[device] = (msg, msg_rm, out0[2], out1[2], w, o0, o1)
    torch.cuda.synchronize()
    assert _eq(res["cpu"], res["cuda"])


@pytest.mark.gpu
def test_dot_tail_kernels_equal_host_twin_past_the_grid_cap():
    bits, n, roles = 128, N_PAST_CAP, [0, 1, 2]
    cross = [_rand((n,), bits, 80 + c) for c in range(3)]
    recv = [[_rand((n,), bits, 90 + 3 * k + c) for c in range(3)] for k in range(3)]
    recv.append([_rand((n,), 64, 99 + c) for c in range(3)])
    res = {}
    for device in ("cpu", "cuda"):
        to = lambda ts: [t.to(device) for t in ts]  # noqa: E731
        r0 = _dot_r0(to(cross), [False, False, True], roles, bits, n, device)
        rmk, rz, rrt, rrm = (to(t) for t in recv)
        res[device] = (r0, _dot_r1(r0[0], rmk, rz, rrt, rrm, roles, bits, n, device))
    torch.cuda.synchronize()
    assert _eq(res["cpu"], res["cuda"])
