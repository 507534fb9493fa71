"""Secure shuffle: the permuted-gather kernel against its torch composition, and ``pm.shuffle``.

(a) ``R.perm_gather`` (the ``k_perm_gather`` kernel) against ``R.perm_gather_torch`` in the
    same process, on the share vectors of a four-slot Z_2^128 buffer holding ``[65536, 16]`` and
    ``[1024, 1024]`` (gathered along axis 0, three slots per launch), in both holder forms of a
    shuffle step: H0 ``a[perm] + b[perm] - m`` and H1 ``a[perm] + p - m``.  p50 of the timed
    calls (device events) and the effective bandwidth over the three reads and one write per
    element.
(b) ``pm.shuffle`` of ``[65536, 16]`` at fixed(24, 40) on LocalMooseRuntime in its default mode
    (a computation with a Shuffle is evaluated eagerly: every evaluation draws a fresh
    permutation), with the kernel and with the composition as the leaf.

Everything is measured twice (``--repeats``); one JSON line per measurement, no threshold.

Usage::

    python benchmarks/shuffle.py [--runs 50] [--warmup 5] [--repeats 2] [--device cuda:0]
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
SHAPES = ((65536, 16), (1024, 1024))
PROGRAM = (65536, 16)


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
    gen = torch.Generator().manual_seed(1)
    for n, inner in SHAPES:
        rnd = lambda: torch.randint(-2 ** 62, 2 ** 62, (4, n, inner, 2), dtype=torch.int64,  # noqa: E731
                                    generator=gen).to(device)
        xbuf, mbuf, pbuf = rnd(), rnd(), rnd()
        x0, x1 = R.RT(xbuf[0:3], 128), R.RT(xbuf[1:4], 128)
        m, p = R.RT(mbuf[0:3], 128), R.RT(pbuf[1:4], 128)
        perm = torch.randperm(n, generator=gen).to(device)
        timer = _time_device if xbuf.is_cuda else _time_host
        cases = {
            "H0": (lambda: R.perm_gather(x0, perm, b=x1, minus=m, axis=0, nb=1),
                   lambda: R.perm_gather_torch(x0, perm, b=x1, minus=m, axis=0, nb=1)),
            "H1": (lambda: R.perm_gather(x1, perm, plus=p, minus=m, axis=0, nb=1),
                   lambda: R.perm_gather_torch(x1, perm, plus=p, minus=m, axis=0, nb=1)),
        }
        moved = 3 * n * inner * 16 * 4  # three slots; three reads and one write per element
        keep, R.SHUFFLE_KERNEL = R.SHUFFLE_KERNEL, True
        try:
            for name, (kernel, torch_) in cases.items():
                assert torch.equal(kernel().data, torch_().data)  # bit for bit
                for path, fn in (("kernel", kernel), ("torch", torch_)):
                    ms = timer(fn, warmup, runs)
                    rec = {"bench": "shuffle.leaf", "form": name, "path": path,
                           "shape": [n, inner], "repeat": repeat, "p50_ms": ms,
                           "gb_per_s": moved / ms / 1e6, "device": str(device)}
                    out.append(rec)
                    print(json.dumps(rec), flush=True)
        finally:
            R.SHUFFLE_KERNEL = keep
    return out


def program():
    alice, bob, carole = (pm.host_placement(n) for n in ROLES)
    rep = pm.replicated_placement("rep", players=[alice, bob, carole])

    @pm.computation
    def prog(x: pm.Argument(placement=alice, vtype=pm.TensorType(pm.float64), shape=PROGRAM)):
        with alice:
            xf = pm.cast(x, dtype=pm.fixed(24, 40))
        with rep:
            y = pm.shuffle(xf)
        with carole:
            return pm.cast(y, dtype=pm.float64)

    x = np.arange(PROGRAM[0] * PROGRAM[1], dtype=np.float64).reshape(PROGRAM) / 8
    return prog, x


def evaluate(device, warmup, runs, repeat):
    out = []
    comp, x = program()
    for leaf_path in ("kernel", "torch"):
        keep, R.SHUFFLE_KERNEL = R.SHUFFLE_KERNEL, leaf_path == "kernel"
        try:
            rt = pm.LocalMooseRuntime(ROLES, device=device)
            got = rt.evaluate_computation(comp, {"x": x})["output_0"]
            order = (got[:, 0] * 8 / PROGRAM[1]).astype(np.int64)
            assert np.array_equal(np.sort(order), np.arange(PROGRAM[0]))
            assert np.array_equal(got, x[order]) and not np.array_equal(got, x)
            ms = _time_host(lambda: rt.evaluate_computation(comp, {"x": x}), warmup, runs)
        finally:
            R.SHUFFLE_KERNEL = keep
        rec = {"bench": "shuffle.program", "program": "shuffle", "leaf": leaf_path,
               "mode": "eager", "shape": list(PROGRAM), "repeat": repeat, "p50_ms": ms,
               "device": str(device)}
        out.append(rec)
        print(json.dumps(rec), flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--device", default=None)
    ap.add_argument("--part", choices=("all", "leaf", "program"), default="all")
    a = ap.parse_args(argv)

    import torch

    device = a.device or ("cuda:0" if torch.cuda.is_available() else "cpu")
    results = []
    for r in range(a.repeats):
        if a.part in ("all", "leaf"):
            results += leaf(device, a.warmup, a.runs, r)
        if a.part in ("all", "program"):
            results += evaluate(device, a.warmup, a.runs, r)
    return results


if __name__ == "__main__":
    main()
