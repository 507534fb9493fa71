"""A share source's zero slot is one zero strip beside the side's residue images instead of
a full zero image (run_crt_asym; k_crt_gemm16's map entry 7): the GEMM reads the same zero
bytes for every modulus and tile from one (modulus, tile) strip, which the prep rewrites on
every call because the workspace is shared with every other CRT product on the stream.

The product from share sources stays bitwise mx_share3_k + mx_gemm_asym: for every owner
slot and share direction (the zero phase lands in a different entry and a different party's
half for each; both sides from a source gives zero x zero on party 2), on a workspace that a
random stack product has just filled, under graph replay, with the 128-column B' tile, and
with MOOSEX_ZERO_STRIP=0 (full zero images, the A/B arm)."""
import json
import os
import subprocess
import sys

import pytest
import torch

from moose_amd.ir.computation import ReplicatedPlacement
from moose_amd.ops import ring as R
from moose_amd.runtime.session import StackedSession

gpu = pytest.mark.gpu

PLC = ReplicatedPlacement(("alice", "bob", "carole"))
FRAC = 23
NX, NY = 0x51, 0x1_0000_0007  # the two sharings' nonces
F64, RING = 2, 0  # kind codes: MX_SHARE_F64, ring data (MX_CROSS_ARITH)
# (M, N, K), 256 x 256 tiles, k-groups of 256.  One tile and one k-group; row padding, two row
# tiles and two column tiles (the strip is read by tiles other than tile 0); two k-groups;
# row padding with two k-groups.
SHAPES = [(256, 256, 256), (300, 512, 256), (256, 256, 512), (300, 256, 512)]


def _bits_of(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def _plain(kind, shape, seed):
    """tests/test_share_prep.py's operands: 0, -0, negatives and the largest magnitudes at the
    start.  float64 at FRAC = 23: +-(2^104 - 2^60) is the largest that encodes exactly,
    +-2^110 and inf saturate, NaN encodes as 0.  Ring data: 0, -1, 2^127 - 1, -2^127 and
    words with every byte 0xff or 0x80."""
    g = torch.Generator().manual_seed(seed)
    n = shape[0] * shape[1]
    if kind == F64:
        x = torch.rand(n, generator=g, dtype=torch.float64) * 2 - 1
        x[n // 2:] *= 2.0 ** 80
        big = 2.0 ** 104 - 2.0 ** 60
        edge = [0.0, -0.0, 1.0, -1.0, 2.0 ** -23, -(2.0 ** -23), 2.0 ** -24, big, -big,
                2.0 ** 110, -(2.0 ** 110), float("inf"), float("-inf"), float("nan")]
        x[:len(edge)] = torch.tensor(edge, dtype=torch.float64)
        return x.reshape(shape).cuda()
    x = torch.randint(-(2 ** 63), 2 ** 63 - 1, (n, 2), generator=g, dtype=torch.int64)
    lo, hi = -(2 ** 63), 2 ** 63 - 1
    edge = [(0, 0), (-1, -1), (-1, hi), (0, lo), (-1, 0), (0, -1), (lo, lo), (hi, hi)]
    x[:len(edge)] = torch.tensor(edge, dtype=torch.int64)  # (low, high) words
    return x.reshape(shape + (2,)).cuda()


def _uniform_stack(shape, seed):
    """A [3, rows, cols] stack of uniformly random 128-bit ring elements."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randint(0, 256, (3 * shape[0] * shape[1] * 16,), generator=g, dtype=torch.uint8)
    return R.RT(raw.view(torch.int64).reshape((3,) + shape + (2,)).cuda(), 128)


class _Poison:
    """A stack product of uniformly random 128-bit data at a shape no smaller than any in
    this file: run on the stream of a share-source product, it leaves random residue bytes
    (and its own GEMM output) all over the workspace that product is about to use -- where
    the full zero image was, and where the strip is."""

    M, K, N = 512, 512, 512

    def __init__(self):
        self.x, self.y = _uniform_stack((self.M, self.K), 31), _uniform_stack((self.K, self.N), 32)
        self.want = None

    def run(self):
        got = _bits_of(R.dot_cross_asym(self.x, None, self.y, None, rolled=True).data)
        if self.want is None:
            self.want = got
        assert torch.equal(got, self.want)  # and the strip path leaves the stack path alone


class _Case:
    """One shape's operands, the share stacks mx_share3_k writes and mx_gemm_asym's products
    on them, each computed once."""

    def __init__(self, mnk, kind):
        self.M, self.N, self.K = mnk
        self.kind = kind
        self.sess = StackedSession("cuda", seed=7)
        self.x, self.y = _plain(kind, (self.M, self.K), 1), _plain(kind, (self.K, self.N), 2)
        self.stacks, self.want = {}, {}

    def args(self, name, j0, d):
        """The arguments of a sharing by owner j0 in direction d (session fused_share_issue)."""
        t, shape, nonce = ((self.x, (self.M, self.K), NX) if name == "x"
                           else (self.y, (self.K, self.N), NY))
        return (self.kind | (R.SHARE_MIRROR if d == 2 else 0), t, FRAC if self.kind == F64 else 0,
                j0, self.sess.key_ptr(PLC, (j0 + d - 1) % 3), nonce, tuple(shape), 128)

    def stack(self, name, j0, d):
        key = (name, j0, d)
        if key not in self.stacks:
            s0, _ = self.sess.fused_share_run(PLC, self.args(name, j0, d))
            self.stacks[key] = s0.v
        return self.stacks[key]

    def reference(self, side, j0, d):
        """mx_gemm_asym on the written shares (the stack side of a one-sided product keeps
        owner 1, direction 1)."""
        xo, yo = ((j0, d) if "x" in side else (1, 1)), ((j0, d) if "y" in side else (1, 1))
        if (xo, yo) not in self.want:
            self.want[xo, yo] = _bits_of(R.dot_cross_asym(self.stack("x", *xo), None,
                                                          self.stack("y", *yo), None,
                                                          rolled=True).data)
        return self.want[xo, yo]

    def product(self, side, j0, d):
        got = R.dot_cross_asym_src(None if "x" in side else self.stack("x", 1, 1),
                                   None if "y" in side else self.stack("y", 1, 1),
                                   self.args("x", j0, d)[:6] if "x" in side else None,
                                   self.args("y", j0, d)[:6] if "y" in side else None,
                                   self.M, self.K, self.N)
        assert got is not None, (side, j0, d)
        assert tuple(got.shape) == (3, self.M, self.N)
        return got

    def check(self, side, j0, d, before=None):
        want = self.reference(side, j0, d)
        if before is not None:
            before()
        assert torch.equal(_bits_of(self.product(side, j0, d).data), want), (side, j0, d)


def _zero_entries(side, j0, d):
    """The images of the side that hold the zero slot (launch_prep_src's phase 3), of
    A = [x0 + x1, x2, x1, x0] / B = [y0 + y1, y1 + y2, y2, y0]."""
    jr, jv = ((j0 + 1) % 3, j0) if d == 2 else (j0, (j0 + 1) % 3)
    slots = {"x": [(0, 1), (2,), (1,), (0,)], "y": [(0, 1), (1, 2), (2,), (0,)]}[side]
    return [e for e, s in enumerate(slots) if jr not in s and jv not in s]


def test_zero_phase_placement():
    """Where the strip is read.  A: one zero entry for every owner -- entry 3 (party 2's
    second half), 2 (party 1's second half) or 1 (party 1's first half and party 2's first
    half).  B: entry 3 (party 2's first half), entry 2 (both second halves), or none when
    slot 1 is the zero slot, which only sums hold."""
    assert [_zero_entries("x", j0, 1) for j0 in range(3)] == [[1], [3], [2]]
    assert [_zero_entries("y", j0, 1) for j0 in range(3)] == [[2], [3], []]
    for side in "xy":
        for j0 in range(3):  # the direction swaps r and x - r, not the zero slot
            assert _zero_entries(side, j0, 2) == _zero_entries(side, j0, 1)


@gpu
@pytest.mark.parametrize("kind", [F64, RING])
@pytest.mark.parametrize("mnk", SHAPES)
def test_bitwise_share_then_gemm(mnk, kind):
    """Source on A only, on B only and on both, every owner slot and both directions."""
    case = _Case(mnk, kind)
    for j0 in range(3):
        for d in (1, 2):
            for side in ("x", "y", "xy"):
                case.check(side, j0, d)


@gpu
@pytest.mark.parametrize("order", [("x", "y", "xy"), ("y", "x", "xy")])
def test_stale_workspace(order):
    """Before every share-source product a random stack product fills the stream's workspace
    (where the full zero image lay and where the strip lies); the product reads zeros only
    if its own prep wrote them."""
    poison = _Poison()
    case = _Case((300, 512, 256), F64)
    for j0 in range(3):
        for side in order:
            case.check(side, j0, 1, before=poison.run)


@gpu
def test_graph_replay():
    """Warm-up, capture, two replays with the random stack product between them: the
    captured prep rewrites the strip at every replay.  Both equal the eager product on the
    same keys (the key slots hold what the seeded session put there)."""
    poison = _Poison()
    case = _Case((256, 256, 256), F64)
    want = case.reference("xy", 0, 1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        poison.run()  # sizes the stream's workspace for both products before the capture
        eager = _bits_of(case.product("xy", 0, 1).data)
    s.synchronize()
    assert torch.equal(eager, want)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = case.product("xy", 0, 1)
    for i in range(2):
        with torch.cuda.stream(s):
            poison.run()
            out.data.zero_()
            g.replay()
        s.synchronize()
        assert torch.equal(_bits_of(out.data), eager), i


def _children(jobs):
    """Fresh processes, started together: [(mode, env changes)] -> their last output lines."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "zero_strip_child.py")
    procs = []
    for mode, env in jobs:
        e = {k: v for k, v in os.environ.items() if k not in ("MOOSEX_ZERO_STRIP",
                                                              "MOOSEX_CRT_KERNEL")}
        e.update(env, PYTHONUNBUFFERED="1")
        procs.append(subprocess.Popen([sys.executable, child, mode], env=e, text=True,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE))
    lines = []
    for p in procs:
        so, se = p.communicate(timeout=300)
        assert p.returncode == 0, (so[-2000:], se[-4000:])
        lines.append(so.strip().splitlines()[-1])
    return lines


@gpu
def test_switch_and_narrow_tile():
    """MOOSEX_ZERO_STRIP=0 and unset reveal the same bits with the same SessionStats, and the
    switched-off arm is itself bitwise share-then-GEMM on the kernel level.
    MOOSEX_CRT_KERNEL=5 takes the 128-column B' tile (k_crt_prep_src<true, 128>, a strip of
    a_nkb * 128 * 64 bytes): (256, 256, 256) is its smallest shape, two column tiles."""
    on, off, off_kernel, narrow = _children([
        ("reveal", {}), ("reveal", {"MOOSEX_ZERO_STRIP": "0"}),
        ("kernel", {"MOOSEX_ZERO_STRIP": "0"}), ("kernel", {"MOOSEX_CRT_KERNEL": "5"})])
    assert json.loads(on) == json.loads(off)
    assert off_kernel == "ok" and narrow == "ok"
