"""Secure group-by sums and cumulative sums: the prefix-sum kernels against their torch
compositions, and ``pm.group_by_sum`` / ``pm.cumsum`` with either as the leaves.

(a) ``R.scan``, ``R.segscan_cross`` and ``R.segscan_apply`` (the ``k_scan`` / ``k_segscan_*``
    kernels) against ``R.*_torch`` in the same process, on the share vectors of a four-slot
    Z_2^128 buffer holding ``[1, 65536, 4]`` (a table column: a long axis of few lines) and
    ``[64, 1024, 4]``; the scan in both directions, the stages at j = 1 and at the last offset.
    p50 of the timed calls (device events).
(b) replayed ``pm.group_by_sum(shuffle=False)`` and eager ``pm.cumsum`` of ``[65536, 4]`` at
    fixed(24, 40) on LocalMooseRuntime, with the kernels and with the compositions as the leaves.

Everything is measured twice (``--repeats``); one JSON line per measurement, no threshold.

Usage::

    python benchmarks/group_by.py [--runs 50] [--warmup 5] [--repeats 2] [--device cuda:0]
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
SHAPES = ((1, 65536, 4), (64, 1024, 4))
TABLE = (65536, 4)


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
    for outer, n, inner in SHAPES:
        xbuf = rnd(4, outer, n, inner)
        x0, x1, x4 = R.RT(xbuf[0:3], 128), R.RT(xbuf[1:4], 128), R.RT(xbuf, 128)
        timer = _time_device if xbuf.is_cuda else _time_host
        cases = {}
        for rev in (False, True):
            g = R.ScanGeom(outer, n, inner, False, rev)
            cases[("scan", "reverse" if rev else "forward")] = (
                lambda g=g: R.scan(x4, g, nb=1), lambda g=g: R.scan_torch(x4, g, nb=1))
        for j in (1, R.segscan_stages(n)[-1]):
            g = R.SegscanGeom(outer, n, inner, j)
            p4 = R.RT(rnd(4, outer, n - j, inner), 128)
            cases[("segscan_cross", f"j={j}")] = (
                lambda g=g: R.segscan_cross(x0, x1, g, nb=1),
                lambda g=g: R.segscan_cross_torch(x0, x1, g, nb=1))
            cases[("segscan_apply", f"j={j}")] = (
                lambda g=g, p4=p4: R.segscan_apply(x4, p4, g, nb=1),
                lambda g=g, p4=p4: R.segscan_apply_torch(x4, p4, g, nb=1))
        for (name, variant), (kernel, torch_) in cases.items():
            assert torch.equal(kernel().data, torch_().data)  # bit for bit
            for path, fn in (("kernel", kernel), ("torch", torch_)):
                ms = timer(fn, warmup, runs)
                rec = {"bench": "group_by.leaf", "leaf": name, "variant": variant, "path": path,
                       "shape": [outer, n, inner], "repeat": repeat, "p50_ms": ms,
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
        def prog(x: pm.Argument(placement=alice, vtype=pm.TensorType(pm.float64), shape=TABLE)):
            with alice:
                xf = pm.cast(x, dtype=dt)
            with rep:
                y = body(xf)
            with carole:
                return pm.cast(y, dtype=pm.float64)

        return prog

    rng = np.random.default_rng(0)
    x = rng.integers(-16 * 256, 16 * 256, size=TABLE) / 256.0
    x[:, 0] = rng.integers(0, 1000, size=TABLE[0]) - 500.0  # about a thousand groups
    return {"group_by_sum": (make(lambda v: pm.group_by_sum(v, by=0, shuffle=False)), x, True),
            "cumsum": (make(lambda v: pm.cumsum(v, axis=0)), x, False)}


def program(device, warmup, runs, repeat):
    out = []
    cuda = str(device).startswith("cuda")
    for name, (comp, x, replayed) in programs().items():
        first = None
        for leaf_path in ("kernel", "torch"):
            keep = R.SCAN_KERNEL, R.SEGSCAN_KERNEL
            R.SCAN_KERNEL = R.SEGSCAN_KERNEL = leaf_path == "kernel"
            try:
                rt = pm.LocalMooseRuntime(ROLES, device=device, use_graphs=cuda and replayed)
                got = rt.evaluate_computation(comp, {"x": x})["output_0"]
                if name == "cumsum":
                    assert np.array_equal(got, np.cumsum(x, axis=0))
                first = got if first is None else first
                assert np.array_equal(got, first)  # exact with either leaf
                ms = _time_host(lambda: rt.evaluate_computation(comp, {"x": x}), warmup, runs)
            finally:
                R.SCAN_KERNEL, R.SEGSCAN_KERNEL = keep
            rec = {"bench": "group_by.program", "program": name, "leaf": leaf_path,
                   "mode": "replay" if cuda and replayed else "eager", "shape": list(x.shape),
                   "repeat": repeat, "p50_ms": ms, "device": str(device)}
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
            results += program(device, a.warmup, a.runs, r)
    return results


if __name__ == "__main__":
    main()
