"""Secure smooth activations: the fused piecewise-polynomial kernel against the torch
composition, and SiLU as one operator against ``x * sigmoid(x)``.

(a) ``R.pwp_cross`` (the ``k_pwp_cross`` kernel) against ``R.pwp_torch`` (weighted sums of the
    flag planes, then elementwise products and sums) in the same process, on the share vectors
    of four-slot Z_2^128 buffers: every power ``[4, 8, 32, 32, 64]`` in a buffer of its own,
    flags ``[4, 8, 8, 32, 32, 64]`` (k = 8), degree 2 and 3.  p50 of the timed calls (device
    events) and the effective GB/s = (bytes read + bytes written) / time with every operand
    counted once per party.
(b) ``pm.silu`` on NHWC ``[8, 32, 32, 64]`` at fixed(24, 40) on LocalMooseRuntime with hipGraph
    replay, against ``pm.mul(x, pm.sigmoid(x))`` in the same process, the operator with the
    kernel and with the composition as the leaf; and the node count of the same programs'
    three-party composed replay (the parties as threads on one GPU).

Everything is measured twice (``--repeats``); one JSON line per measurement, no threshold.

Usage::

    python benchmarks/smooth_activation.py [--runs 50] [--warmup 5] [--repeats 2]
                                           [--device cuda:0] [--part all|leaf|silu|nodes]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import moose_amd as pm  # noqa: E402
from moose_amd.ops import ring as R  # noqa: E402

ROLES = ["alice", "bob", "carole"]
IMAGE = (8, 32, 32, 64)
K = 8


def _time_device(fn, warmup, runs):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    lat = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        lat.append(e0.elapsed_time(e1))
    lat.sort()
    return lat[len(lat) // 2]


def _time_host(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    lat = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        lat.append((time.perf_counter() - t0) * 1e3)
    lat.sort()
    return lat[len(lat) // 2]


def leaf(device, warmup, runs, repeat):
    import torch

    out = []
    rnd = lambda *s: torch.randint(-2 ** 62, 2 ** 62, s + (2,), dtype=torch.int64,  # noqa: E731
                                   device=device)
    for d in (2, 3):
        sbuf = rnd(4, K, *IMAGE)
        pbufs = [rnd(4, *IMAGE) for _ in range(d)]
        s0, s1 = R.RT(sbuf[0:3], 128), R.RT(sbuf[1:4], 128)
        p0 = [R.RT(b[0:3], 128) for b in pbufs]
        p1 = [R.RT(b[1:4], 128) for b in pbufs]
        D = [[((-1) ** j * (j + 3 + i)) << (80 if i == 0 else 37) for j in range(K)]
             for i in range(d + 1)]
        CK = [(i + 1) << 39 for i in range(d)]
        args = (s0, s1, p0, p1, D, CK)
        timer = _time_device if sbuf.is_cuda else _time_host
        kernel = lambda: R.pwp_cross(*args, nb=1)  # noqa: E731
        torch_ = lambda: R.pwp_torch(*args, nb=1)  # noqa: E731
        got = kernel()
        assert torch.equal(got.data, torch_().data)  # bit for bit
        one = lambda t: R.RT(t.data[1:2].cpu(), 128)  # noqa: E731
        want = R.pwp_cross(one(s0), one(s1), [one(t) for t in p0], [one(t) for t in p1], D, CK,
                           nb=1)
        assert torch.equal(got.data[1:2].cpu(), want.data)  # and the CPU twin, on one slot
        n = 3 * int(np.prod(IMAGE))
        nbytes = 16 * n * (2 * K + 2 * d + 1)
        for path, fn in (("kernel", kernel), ("torch", torch_)):
            ms = timer(fn, warmup, runs)
            rec = {"bench": "pwp.leaf", "path": path, "k": K, "degree": d, "image": list(IMAGE),
                   "repeat": repeat, "p50_ms": ms, "gbps": nbytes / ms / 1e6,
                   "device": str(device)}
            out.append(rec)
            print(json.dumps(rec), flush=True)
    return out


def programs():
    alice, bob, carole = (pm.host_placement(n) for n in ROLES)
    rep = pm.replicated_placement("rep", players=[alice, bob, carole])
    dt = pm.fixed(24, 40)

    def make(body):
        @pm.computation
        def prog(x: pm.Argument(placement=alice, vtype=pm.TensorType(pm.float64))):
            with alice:
                xf = pm.cast(x, dtype=dt)
            with rep:
                y = body(xf)
            with carole:
                return pm.cast(y, dtype=pm.float64)

        return prog

    return {"operator": make(lambda x: pm.silu(x)),
            "composed": make(lambda x: pm.mul(x, pm.sigmoid(x)))}


def silu(device, warmup, runs, repeat):
    from moose_amd.protocols import fixedpoint as fxp

    out = []
    x = np.random.default_rng(0).uniform(-8, 8, IMAGE)
    want = x / (1 + np.exp(-x))
    fit = fxp.smooth_tables("silu", 1.0, 3, 8, 40)[2]
    cuda = str(device).startswith("cuda")
    for name, comp in programs().items():
        for leaf_path in (("kernel", "torch") if name == "operator" else ("kernel",)):
            R.PWP_KERNEL = leaf_path == "kernel"
            try:
                rt = pm.LocalMooseRuntime(ROLES, device=device, use_graphs=cuda)
                got = rt.evaluate_computation(comp, {"x": x})["output_0"]
                err = float(np.abs(got - want).max())
                # the operator: its fit error; the composition: what the sigmoid keeps, times 8
                assert err <= (fit + 64 * 2.0 ** -40 if name == "operator" else 2e-5), err
                ms = _time_host(lambda: rt.evaluate_computation(comp, {"x": x}), warmup, runs)
            finally:
                R.PWP_KERNEL = True
            rec = {"bench": "pwp.silu", "program": name, "leaf": leaf_path,
                   "mode": "replay" if cuda else "eager", "image": list(IMAGE),
                   "repeat": repeat, "p50_ms": ms, "max_abs_err": err, "device": str(device)}
            out.append(rec)
            print(json.dumps(rec), flush=True)
    return out


def nodes(device, warmup, runs):
    """The kernel count of each program's graph: the stacked runtime's captured graphs expose
    none, so it is taken with the three parties as threads on this GPU, whose tapes are
    composed into one hipGraph that reports its nodes."""
    out = []
    x = np.random.default_rng(0).uniform(-8, 8, IMAGE)
    for name, comp in programs().items():
        rt = pm.LocalMooseRuntime(ROLES, device_map={r: device for r in ROLES},
                                  use_graphs=True, timeout=60)
        ms = _time_host(lambda: rt.evaluate_computation(comp, {"x": x}), warmup, runs)
        tapes = [t for _, t in rt._party_tapes.values() if t]
        gn = (tapes[0].graph_nodes or {}) if tapes else {}
        rec = {"bench": "pwp.silu", "program": name, "mode": "parties_replay", "p50_ms": ms,
               "device": str(device), "replayed": bool(tapes), "nodes": gn.get("nodes"),
               "party_batched": gn.get("party_batched")}
        out.append(rec)
        print(json.dumps(rec), flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--device", default=None)
    ap.add_argument("--part", choices=("all", "leaf", "silu", "nodes"), default="all")
    a = ap.parse_args(argv)

    import torch

    device = a.device or ("cuda:0" if torch.cuda.is_available() else "cpu")
    results = []
    for r in range(a.repeats):
        if a.part in ("all", "leaf"):
            results += leaf(device, a.warmup, a.runs, r)
        if a.part in ("all", "silu"):
            results += silu(device, a.warmup, a.runs, r)
    if a.part in ("all", "nodes") and str(device).startswith("cuda"):
        results += nodes(device, a.warmup, a.runs)
    return results


if __name__ == "__main__":
    main()
