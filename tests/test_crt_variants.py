"""The CRT GEMM's variant table, reconstruction forms and return codes (csrc/gemm_crt.hip).

MOOSEX_CRT_KERNEL names one of six kernel variants (5, 6, 8, 12, 14, 16); every other value --
a retired id, 0, 17, text -- selects 8.  One record decides the B' tile width of the plan and
the kernel that is launched, so the two cannot disagree: under every value the plain cross
GEMM, the rolled pair and the asymmetric product equal the limb GEMM bitwise on the smallest
shape that crosses a tile edge in both directions with a ragged last tile (M = 300, N = 280,
K = 320, both rings).  MOOSEX_CRT_RECON is cached at first use, so the multiply-add
reconstruction runs in fresh child processes (tests/crt_variants_child.py).  The return codes
of the entry points where a product does not apply are those recorded from the commit before
the variants were retired; every one of them is answered before any launch."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from moose_amd.ops import native as nat
from moose_amd.ops import ring as R

gpu = pytest.mark.gpu

M, N, K = 300, 280, 320  # tests/test_gemm_crt.py's test_gpu_dot_cross_pair_rolled
LIVE = ["5", "6", "8", "12", "14", "16"]
STRAY = ["1", "3", "4", "7", "15", "0", "17", "x"]


def rand_rt(shape, bits, seed):
    g = torch.Generator().manual_seed(seed)
    d = torch.randint(-(2**63), 2**63 - 1, shape + ((2,) if bits == 128 else ()), generator=g,
                      dtype=torch.int64)
    return R.RT(d.cuda(), bits)


class _crt:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        nat.lib().mx_set_gemm_crt(self.mode)

    def __exit__(self, *a):
        nat.lib().mx_set_gemm_crt(0)


def _rolled(t):
    return R.RT(torch.roll(t.data, -1, dims=0).contiguous(), t.bits)


def _bcast(t, k=2):
    d = t.data.unsqueeze(1)
    return R.RT(d.expand((3, k) + tuple(d.shape[2:])), t.bits)


class Case:
    """One ring's operands and their limb-GEMM products, computed once and left unchanged."""

    def __init__(self, bits):
        self.bits = bits
        self.x0 = rand_rt((3, M, K), bits, 210)
        self.x1 = _rolled(self.x0)
        self.ys = [rand_rt((3, K, N), bits, 211 + i) for i in range(2)]
        self.y0, self.y1 = self.ys[0], _rolled(self.ys[0])
        # the asymmetric product's short form: the first 64 of the K columns / rows
        self.xs0 = R.RT(self.x0.data[:, :, :64].contiguous(), bits)
        self.ys0 = R.RT(self.y0.data[:, :64].contiguous(), bits)
        with _crt(2):
            self.cross = R.dot_cross(self.x0, self.x1, *self.ys, nb=1)
            self.asym = R.dot_cross(*R._asym_operands(self.x0, self.x1, self.y0, self.y1), nb=1)
            self.asym64 = R.dot_cross(*R._asym_operands(self.xs0, _rolled(self.xs0), self.ys0,
                                                        _rolled(self.ys0)), nb=1)
            self.bc = R.dot_cross(_bcast(self.x0), _bcast(self.x1), _bcast(self.ys[0]),
                                  _bcast(self.ys[1]), nb=2)

    def check(self, broadcast=False):
        """The three CRT products (and the batch-broadcast one) against the limb GEMM."""
        with _crt(1):
            cross = R.dot_cross(self.x0, self.x1, *self.ys, nb=1)
            pair = R.dot_cross_pair(self.x0, self.ys[0], self.ys[1], 1)
            asym = R.dot_cross_asym(self.x0, None, self.y0, None, rolled=True)
            asym64 = R.dot_cross_asym(self.xs0, None, self.ys0, None, rolled=True)
            bc = (R.dot_cross(_bcast(self.x0), _bcast(self.x1), _bcast(self.ys[0]),
                              _bcast(self.ys[1]), nb=2) if broadcast else None)
        assert pair is not None
        for name, got, want in (("cross", cross, self.cross), ("pair", pair, self.cross),
                                ("asym", asym, self.asym), ("asym64", asym64, self.asym64)):
            assert torch.equal(got.data, want.data), name
        if broadcast:
            assert torch.equal(bc.data, self.bc.data), "broadcast"


_CASES = {}


def case(bits):
    if bits not in _CASES:
        _CASES[bits] = Case(bits)
    return _CASES[bits]


@gpu
@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("value", STRAY)
def test_retired_and_stray_values_select_8(value, bits, monkeypatch):
    """A value without a record must not reach a kernel of another tile width than the plan's:
    the products stay those of the limb GEMM."""
    monkeypatch.setenv("MOOSEX_CRT_KERNEL", value)
    case(bits).check()


@gpu
@pytest.mark.parametrize("bits", [64, 128])
@pytest.mark.parametrize("variant", LIVE)
def test_live_variants_small_shape(variant, bits, monkeypatch):
    """Every live id where the last tile is ragged in both directions; 5 (128-column tiles)
    and 8 also with both operands broadcast over a batch (a_bstride = b_bstride = 0)."""
    monkeypatch.setenv("MOOSEX_CRT_KERNEL", variant)
    case(bits).check(broadcast=variant in ("5", "8"))


# --- reconstruction forms: fresh processes ------------------------------------------------------
def _child(env):
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "crt_variants_child.py")
    e = {k: v for k, v in os.environ.items() if k not in ("MOOSEX_CRT_RECON",
                                                          "MOOSEX_CRT_KERNEL")}
    e.update(env, PYTHONUNBUFFERED="1")
    p = subprocess.run([sys.executable, child], env=e, text=True, capture_output=True,
                       timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    return json.loads(p.stdout.strip().splitlines()[-1])


@gpu
def test_reconstruction_forms():
    """MOOSEX_CRT_RECON=0 (multiply-add) under the 256- and the 128-column tile: the products,
    an accumulate into a non-zero C included, equal the limb GEMM, and a product cannot stop at
    its residues (-7 from mx_crt_defer_bytes and from mx_gemm_asym with ``residues``).  The
    default form defers under 256-column tiles (a positive byte count: 3 parties x n moduli x
    2 x 2 tiles of 256 x 256 bytes) and not under 128-column ones."""
    n = {64: nat.lib().mx_crt_moduli(1, 2 * K), 128: nat.lib().mx_crt_moduli(2, 2 * K)}
    full = {str(b): 3 * n[b] * 4 * 256 * 256 for b in (64, 128)}
    no = {"64": -7, "128": -7}
    for env, defer, rc in (({"MOOSEX_CRT_RECON": "0", "MOOSEX_CRT_KERNEL": "8"}, no, no),
                           ({"MOOSEX_CRT_RECON": "0", "MOOSEX_CRT_KERNEL": "5"}, no, no),
                           ({"MOOSEX_CRT_KERNEL": "8"}, full, {"64": 0, "128": 0}),
                           ({"MOOSEX_CRT_KERNEL": "5"}, no, no)):
        got = _child(env)
        print(env, got)
        assert got["products"] == "ok", env
        assert got["defer_bytes"] == defer, env
        assert got["asym_residues_rc"] == rc, env


# --- return codes ---------------------------------------------------------------------------------
def _entry_points():
    h = nat.lib()
    i, q, p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    for name, res, args in (
            ("mxh_crt_recon_open", i, [i, p, p, q, p, i, p, i, p]),
            ("mxh_crt_roll", i, [i, q, q, q, q, p, q, q, p, p, p, p, i, p])):
        fn = getattr(h, name)
        fn.restype, fn.argtypes = res, args
    return h


def return_codes():
    """(entry point, condition) -> code.  No operand is read: each call is answered before any
    launch, so ``buf`` only stands for a pointer that is not null."""
    h = _entry_points()
    buf = np.zeros(64, np.int64)
    P = buf.ctypes.data
    out = {}

    def entries(tag, words, m, n_, k):
        crt = (ctypes.c_int64 * 4)(P, m, n_, k)
        out["gemm_asym", tag] = h.mx_gemm_asym(words, m, n_, k, P, None, P, None, 1, P, None, None)
        out["gemm_asym_res", tag] = h.mx_gemm_asym(words, m, n_, k, P, None, P, None, 1, None,
                                                   None, P)
        out["gemm_asym_src", tag] = h.mx_gemm_asym_src(words, m, n_, k, P, P, None, None, P, None,
                                                       None)
        out["gemm_asym_src_res", tag] = h.mx_gemm_asym_src(words, m, n_, k, P, P, None, None,
                                                           None, None, P)
        out["defer_bytes", tag] = h.mx_crt_defer_bytes(words, m, n_, k)
        out["recon_open", tag] = h.mxh_crt_recon_open(words, crt, P, m * n_, P, 20, P, 23, None)
        return crt

    for w in (1, 2):
        entries(f"K=96,w{w}", w, 256, 256, 96)
        out["recon", f"K=96,w{w}"] = h.mx_crt_recon(w, 256, 256, 96, P, P, None)
        out["roll", f"K=96,w{w}"] = h.mxh_crt_roll(w, 3, 256, 256, 96, P, 256 * 96, 1, P, P, None,
                                                  P, 0, None)
        entries(f"K=16448,w{w}", w, 1, 1, 16448)
        out["recon", f"K=16448,w{w}"] = h.mx_crt_recon(w, 1, 1, 16448, P, P, None)
        out["roll", f"K=16448,w{w}"] = h.mxh_crt_roll(w, 3, 1, 1, 16448, P, 16448, 1, P, P, None,
                                                     P, 0, None)
        entries(f"M=0,w{w}", w, 0, 256, 256)
        out["gemm_asym", f"S1=null,w{w}"] = h.mx_gemm_asym(w, 256, 256, 256, P, None, P, None, 0,
                                                           P, None, None)
        out["roll", f"batch=1,w{w}"] = h.mxh_crt_roll(w, 1, 256, 256, 256, P, 256 * 256, 1, P, P,
                                                     None, P, 0, None)
        out["roll", f"roll%batch=0,w{w}"] = h.mxh_crt_roll(w, 3, 256, 256, 256, P, 256 * 256, 3,
                                                          P, P, None, P, 0, None)
    entries("words=3", 3, 256, 256, 256)
    out["recon", "words=3"] = h.mx_crt_recon(3, 256, 256, 256, P, P, None)
    out["roll", "words=3"] = h.mxh_crt_roll(3, 3, 256, 256, 256, P, 256 * 256, 1, P, P, None, P, 0,
                                            None)
    return out


def _both(d):
    return {(e, f"{c},w{w}"): v for (e, c), v in d.items() for w in (1, 2)}


# recorded from the commit before this file existed (the same for both rings)
PARENT_CODES = {
    **_both({("gemm_asym", "K=96"): -7, ("gemm_asym_res", "K=96"): -7,
             ("gemm_asym_src", "K=96"): -7, ("gemm_asym_src_res", "K=96"): -7,
             ("gemm_asym_src_res", "K=16448"): -6, ("gemm_asym_src_res", "M=0"): -7,
             ("defer_bytes", "K=96"): -7,
             ("recon_open", "K=96"): -7, ("recon", "K=96"): -7, ("roll", "K=96"): -7,
             ("gemm_asym", "K=16448"): -6, ("gemm_asym_res", "K=16448"): -6,
             ("gemm_asym_src", "K=16448"): -6, ("defer_bytes", "K=16448"): -7,
             ("recon_open", "K=16448"): -7, ("recon", "K=16448"): -7, ("roll", "K=16448"): -6,
             ("gemm_asym", "M=0"): 0, ("gemm_asym_res", "M=0"): -7,
             ("gemm_asym_src", "M=0"): 0, ("defer_bytes", "M=0"): -7, ("recon_open", "M=0"): -3,
             ("gemm_asym", "S1=null"): -2, ("roll", "batch=1"): -7,
             ("roll", "roll%batch=0"): -7}),
    ("gemm_asym", "words=3"): -2, ("gemm_asym_res", "words=3"): -2,
    ("gemm_asym_src", "words=3"): -7, ("gemm_asym_src_res", "words=3"): -7,
    ("defer_bytes", "words=3"): -7,
    ("recon_open", "words=3"): -7, ("recon", "words=3"): -7, ("roll", "words=3"): -2,
}
# mx_gemm_asym_src takes Z_2^128 only: -7 for Z_2^64 whatever the sizes
PARENT_CODES.update({(e, f"{c},w1"): -7 for c in ("K=96", "K=16448")
                     for e in ("gemm_asym_src", "gemm_asym_src_res")})


def test_return_codes_are_the_parents():
    got = return_codes()
    print(sorted(got.items()))
    assert got == PARENT_CODES
