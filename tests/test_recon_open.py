"""A revealed stacked dot reconstructs its CRT product inside the opening kernel
(k_crt_recon16d_open; ring.CrtProduct, mx_mul_trunc3_open's crt form): the product stops at the
GEMM's output residues and the opening rebuilds the three parties' products, adds them and
applies mxf::trunc_pr_open -- the opened value of the tail's new sharing from the products' sum
and r0 + r1 alone.

The output must be bitwise the two kernels it replaces (k_crt_recon16d, then
k_mul_trunc3_open on the same keys and nonces) on the same residue buffer, at ragged shapes,
for every owner slot of share-source operands, after a random product has filled the GEMM
workspace, under graph replay, and through a session with MOOSEX_DOT_OPEN_FUSED on and off
and on the host; shares read after the opening come from the ordinary tail, same bits."""
import random

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

gpu = pytest.mark.gpu

PLC = ReplicatedPlacement(("alice", "bob", "carole"))
NMUL, NONCES = 0x1234, (11, 12, 13, 14, 15, 16)
FRAC = 23
F64 = 2  # kind code MX_SHARE_F64
NX, NY = 0x51, 0x1_0000_0007
# (M, N, K); tiles are 256 x 256, the opening kernel's strip is 8 rows x one tile's columns.
# One tile.  Ragged last tiles both ways, N no multiple of 64: rows of the flat keystream
# order start in the middle of a ChaCha block group, a 1-row last strip, a 44-column last
# tile.  Several tiles per strip row, two row tiles.  Fewer elements than one strip.
SHAPES = [(256, 256, 256), (257, 300, 256), (512, 768, 320), (5, 100, 64)]


def _bits_of(t):
    return t.detach().cpu().contiguous().view(torch.int64)


# -- the algebra, on integers ------------------------------------------------------------------
def _z1(W, x, r0, r1, rt0, rm0, z0, z2, m):
    """mxf::trunc_pr_z1 over Z_2^W."""
    mask, k = (1 << W) - 1, W - 1
    r = (r0 + r1) & mask
    r_msb, r_top = r >> (W - 1), ((r << 1) & mask) >> (m + 1)
    rt1, rm1 = r_top - rt0, r_msb - rm0
    c = (x[0] + x[1] + (1 << (k - 1)) + r0 + x[2] + r1) & mask
    c_msb, c_top = c >> (W - 1), ((c << 1) & mask) >> (m + 1)
    ov0 = rm0 - 2 * c_msb * rm0 + c_msb
    y0 = (ov0 << (k - m)) - rt0 + c_top - (1 << (k - 1 - m))
    ov1 = rm1 - 2 * c_msb * rm1
    y1 = (ov1 << (k - m)) - rt1
    return ((y0 - z0) + (y1 - z2)) & mask


def _open(W, xsum, r, m):
    """mxf::trunc_pr_open over Z_2^W."""
    mask, k = (1 << W) - 1, W - 1
    r_msb, r_top = r >> (W - 1), ((r << 1) & mask) >> (m + 1)
    c = (xsum + (1 << (k - 1)) + r) & mask
    c_msb, c_top = c >> (W - 1), ((c << 1) & mask) >> (m + 1)
    ov = r_msb - 2 * c_msb * r_msb + c_msb
    return ((ov << (k - m)) - r_top + c_top - (1 << (k - 1 - m))) & mask


@pytest.mark.parametrize("W", [64, 128])
def test_opened_sum_needs_the_product_sum_and_r_only(W):
    """z0 + z1 + z2 of the tail (zero share on the products, then TruncPr) equals
    trunc_pr_open(sum of the products, r0 + r1): the zero share's three streams, rt0, rm0, z0
    and z2 cancel bit for bit -- at random values and at the ring's edges."""
    rng = random.Random(W)
    mask = (1 << W) - 1
    edges = [0, 1, mask, 1 << (W - 1), (1 << (W - 1)) - 1, 1 << (W - 2)]
    for trial in range(400):
        draw = lambda: rng.choice(edges) if rng.random() < 0.3 else rng.getrandbits(W)  # noqa: E731
        v, ks = [draw() for _ in range(3)], [draw() for _ in range(3)]
        r0, r1, rt0, rm0, z0, z2 = (draw() for _ in range(6))
        m = rng.choice([1, 23, 40, 63, 126] if W == 128 else [1, 23, 62])
        x = [(v[p] + ks[p] - ks[(p + 1) % 3]) & mask for p in range(3)]
        want = (z0 + _z1(W, x, r0, r1, rt0, rm0, z0, z2, m) + z2) & mask
        assert _open(W, sum(v) & mask, (r0 + r1) & mask, m) == want, trial


# -- kernel level ----------------------------------------------------------------------------
def _uniform_stack(shape, bits, seed):
    """A [3, rows, cols] stack of uniformly random ring elements."""
    g = torch.Generator().manual_seed(seed)
    nb = bits // 8
    raw = torch.randint(0, 256, (3 * shape[0] * shape[1] * nb,), generator=g, dtype=torch.uint8)
    shp = (3,) + shape + ((2,) if bits == 128 else ())
    return R.RT(raw.view(torch.int64).reshape(shp).cuda(), bits)


def _deferred(x, y):
    with R.deferred_products():
        z = R.dot_cross_asym(x, None, y, None, rolled=True)
    assert isinstance(z, R.CrtProduct) and z.pending()
    return z


def _two_kernels(z, slot, m):
    """k_crt_recon16d on the product's residues (its ``data``), then k_mul_trunc3_open."""
    dense = R.RT(z.data, z.bits)
    assert not z.pending()
    return R.zs_trunc3_open(dense, slot, NMUL, m, NONCES, FRAC)


@gpu
@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("mnk", SHAPES)
def test_fused_entry_matches_recon_then_open(mnk, bits):
    M, N, K = mnk
    sess = StackedSession("cuda", seed=7)
    slot = sess.key_ptr(PLC, 0)
    x, y = _uniform_stack((M, K), bits, 1), _uniform_stack((K, N), bits, 2)
    plain = _bits_of(R.dot_cross_asym(x, None, y, None, rolled=True).data)
    z = _deferred(x, y)
    got = {}
    for m in [1, 23, 63] + ([40] if bits == 128 else []):
        got[m] = z.open(slot, NMUL, m, NONCES, FRAC)
        assert z.pending() and got[m].dtype == torch.float64 and tuple(got[m].shape) == (M, N)
    # the reconstruction the product skipped: bitwise the ordinary product
    assert torch.equal(_bits_of(z.data), plain)
    for m, g in got.items():
        assert torch.equal(_bits_of(g), _bits_of(_two_kernels(z, slot, m))), m


class _Poison:
    """A stack product of random data no smaller than any source case here, run on the
    stream: it leaves its residues all over the GEMM workspace."""

    def __init__(self):
        self.x, self.y = _uniform_stack((512, 512), 128, 31), _uniform_stack((512, 512), 128, 32)

    def run(self):
        return R.dot_cross_asym(self.x, None, self.y, None, rolled=True).data


class _Sources:
    """Float operands shared inside the product's prep (mx_gemm_asym_src), as a session's
    fresh inputs are."""

    def __init__(self, mnk):
        self.M, self.N, self.K = mnk
        self.sess = StackedSession("cuda", seed=7)
        g = torch.Generator().manual_seed(5)
        self.x = (torch.rand((self.M, self.K), generator=g, dtype=torch.float64) * 2 - 1).cuda()
        self.y = (torch.rand((self.K, self.N), generator=g, dtype=torch.float64) * 2 - 1).cuda()

    def args(self, name, j0, d):
        t, nonce = (self.x, NX) if name == "x" else (self.y, NY)
        return (F64 | (R.SHARE_MIRROR if d == 2 else 0), t, FRAC, j0,
                self.sess.key_ptr(PLC, (j0 + d - 1) % 3), nonce)

    def product(self, j0, d, defer):
        with R.deferred_products(defer):
            z = R.dot_cross_asym_src(None, None, self.args("x", j0, d), self.args("y", j0, d),
                                     self.M, self.K, self.N)
        assert z is not None and isinstance(z, R.CrtProduct) == defer
        return z

    def slot(self):
        return self.sess.key_ptr(PLC, 0)


@gpu
@pytest.mark.parametrize("mnk", [(256, 256, 256), (300, 512, 256)])
def test_every_owner_slot(mnk):
    """Both operands from share sources, every owner slot and both directions (the zero
    strip lands in a different image for each)."""
    src = _Sources(mnk)
    for j0 in range(3):
        for d in (1, 2):
            want = R.zs_trunc3_open(src.product(j0, d, False), src.slot(), NMUL, 23, NONCES, FRAC)
            got = src.product(j0, d, True).open(src.slot(), NMUL, 23, NONCES, FRAC)
            assert torch.equal(_bits_of(got), _bits_of(want)), (j0, d)


@gpu
def test_after_a_random_product_filled_the_workspace():
    """The residues are the product's own buffer: a product that runs between the GEMM and
    the opening, and one before the GEMM, change nothing."""
    poison, src = _Poison(), _Sources((300, 512, 256))
    want = R.zs_trunc3_open(src.product(1, 1, False), src.slot(), NMUL, 23, NONCES, FRAC)
    poison.run()
    z = src.product(1, 1, True)
    poison.run()
    assert torch.equal(_bits_of(z.open(src.slot(), NMUL, 23, NONCES, FRAC)), _bits_of(want))


@gpu
def test_graph_replay():
    """Warm-up, capture of product + opening, two replays with the random product between
    them: each equals the eager two-kernel result on the same keys."""
    poison, src = _Poison(), _Sources((256, 256, 256))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        poison.run()  # sizes the stream's workspace before the capture
        want = _bits_of(R.zs_trunc3_open(src.product(0, 1, False), src.slot(), NMUL, 23, NONCES,
                                         FRAC))
        eager = _bits_of(src.product(0, 1, True).open(src.slot(), NMUL, 23, NONCES, FRAC))
    s.synchronize()
    assert torch.equal(eager, want)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = src.product(0, 1, True).open(src.slot(), NMUL, 23, NONCES, FRAC)
    for i in range(2):
        with torch.cuda.stream(s):
            poison.run()
            out.zero_()
            g.replay()
        s.synchronize()
        assert torch.equal(_bits_of(out), want), i


# -- through the runtime ---------------------------------------------------------------------
alice, bob, carole = (pm.host_placement(n) for n in ("alice", "bob", "carole"))
replicated = pm.replicated_placement("rep", players=[alice, bob, carole])
FX = pm.fixed(14, 23)
F64T = pm.TensorType(pm.float64)


def _dot_reveal():
    @pm.computation
    def comp(x: pm.Argument(placement=alice, vtype=F64T),
             y: pm.Argument(placement=bob, vtype=F64T)):
        with alice:
            xf = pm.cast(x, dtype=FX)
        with bob:
            yf = pm.cast(y, dtype=FX)
        with replicated:
            z = pm.dot(xf, yf)
        with carole:
            out = pm.cast(z, dtype=pm.float64)
        return out

    return comp


class _Calls:
    NAMES = ("mx_mul_trunc3_open", "mx_crt_recon", "mx_mul_trunc3_kv")

    def __init__(self, monkeypatch):
        self.n = {k: 0 for k in self.NAMES}
        self.crt = 0  # openings given residues
        lib = nat.lib()
        for name in self.NAMES:
            monkeypatch.setattr(lib, name, self._wrap(name, getattr(lib, name)), raising=False)

    def _wrap(self, name, fn):
        def call(*a):
            self.n[name] += 1
            if name == "mx_mul_trunc3_open" and a[-1] is not None:
                self.crt += 1
            return fn(*a)

        return call


def _run(args, ring, monkeypatch, calls, fused, device="cuda:0"):
    """Output, stats and the launches of this run: (counts by name, openings given residues)."""
    monkeypatch.setenv("MOOSEX_DOT_OPEN_FUSED", "1" if fused else "0")  # read at every dot
    n0, crt0 = dict(calls.n), calls.crt
    rt = pm.LocalMooseRuntime(["alice", "bob", "carole"], device=device, seed=21,
                              use_graphs=False, fixedpoint_ring=ring)
    out = rt.evaluate_computation(_dot_reveal(), args)["output_0"]
    return (np.asarray(out), rt.last_stats.as_dict(),
            ({k: calls.n[k] - n0[k] for k in n0}, calls.crt - crt0))


@gpu
@pytest.mark.parametrize("ring", [64, 128])
@pytest.mark.parametrize("mnk", SHAPES[:3])
def test_session_dot_reveal_switch_and_host(mnk, ring, monkeypatch):
    M, N, K = mnk
    rng = np.random.default_rng(5)
    args = {"x": rng.uniform(-1, 1, (M, K)), "y": rng.uniform(-1, 1, (K, N))}
    calls = _Calls(monkeypatch)
    on, st_on, c_on = _run(args, ring, monkeypatch, calls, True)
    off, st_off, c_off = _run(args, ring, monkeypatch, calls, False)
    host, _, _ = _run(args, ring, monkeypatch, calls, True, device="cpu")
    assert np.array_equal(on.view(np.int64), off.view(np.int64))
    assert np.array_equal(on.view(np.int64), host.view(np.int64))
    for k in ("rounds", "reshare_bytes", "bytes", "messages"):
        assert st_on[k] == st_off[k], k
    # one opening either way; given residues when switched on, and no reconstruction launch
    assert c_on == ({"mx_mul_trunc3_open": 1, "mx_crt_recon": 0, "mx_mul_trunc3_kv": 0}, 1)
    assert c_off == (c_on[0], 0)
    assert np.abs(on - args["x"] @ args["y"]).max() < 1e-4


@gpu
def test_shares_read_after_the_opening(monkeypatch):
    """The value is opened from the residues, then its shares are read: the reconstruction
    and the ordinary tail run then, on the same keys and nonces -- the shares and the opened
    value are those of the switched-off run, and the shares sum to the opened value."""
    bits, M = 128, 256
    outs = []
    for fused in ("1", "0"):
        monkeypatch.setenv("MOOSEX_DOT_OPEN_FUSED", fused)
        sess = StackedSession("cuda", seed=3)
        x0, y0 = _uniform_stack((M, M), bits, 1), _uniform_stack((M, M), bits, 2)
        roll = lambda t: R.RT(torch.roll(t.data, -1, dims=0).contiguous(), bits)  # noqa: E731
        X = rep.RepTensor(PLC, bits, "arith", PV(PLC, x0), PV(PLC, roll(x0)))
        Y = rep.RepTensor(PLC, bits, "arith", PV(PLC, y0), PV(PLC, roll(y0)))
        z = rep.dot_trunc(sess, X, Y, 23)
        assert isinstance(z, rep.StackedTail) and rep.lazy(z)
        assert isinstance(z.v.v, R.CrtProduct) == (fused == "1")
        out = R.decode(rep.reveal(sess, z, "carole").v, 23)
        assert not z.done
        s0, s1 = z.s0.v, z.s1.v
        sums = R.decode(R.opened(R.RT(s0.data[2], bits), R.RT(s1.data[2], bits),
                                 R.RT(s1.data[0], bits)), 23)
        assert torch.equal(_bits_of(out), _bits_of(sums))
        outs.append((_bits_of(out), _bits_of(s0.data), _bits_of(s1.data)))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
