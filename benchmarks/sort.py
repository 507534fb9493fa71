"""Secure sorting: the compare-exchange kernels against their torch compositions, and replayed
``pm.sort`` / ``pm.sort_rows`` with either as the leaves.

(a) ``R.cswap_diff``, ``R.cswap_cross`` and ``R.cswap_apply`` (the ``k_cswap_*`` kernels)
    against ``R.cswap_*_torch`` in the same process, on the share vectors of a four-slot
    Z_2^128 buffer holding ``[64, 1024]`` (sorted along the last axis), at the stages j = 1 and
    j = n/2.  p50 of the timed calls (device events).
(b) ``pm.sort`` of ``[64, 1024]`` and ``pm.sort_rows`` of ``[4096, 4]`` at fixed(24, 40) on
    LocalMooseRuntime with hipGraph replay, with the kernels and with the compositions as the
    leaves; and the same programs with the three parties as threads on one GPU (graph node
    count and p50).

Everything is measured twice (``--repeats``); one JSON line per measurement, no threshold.

Usage::

    python benchmarks/sort.py [--runs 50] [--warmup 5] [--repeats 2] [--device cuda:0]
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
SORT, ROWS = (64, 1024), (4096, 4)


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
    outer, n = SORT
    rnd = lambda *s: torch.randint(-2 ** 62, 2 ** 62, s + (2,), dtype=torch.int64,  # noqa: E731
                                   device=device)
    xbuf, sbuf, pbuf = rnd(4, outer, n), rnd(4, outer, n // 2, 1), rnd(4, outer, n // 2, 1)
    x0, x1 = R.RT(xbuf[0:3], 128), R.RT(xbuf[1:4], 128)
    s0, s1 = R.RT(sbuf[0:3], 128), R.RT(sbuf[1:4], 128)
    x4, p4 = R.RT(xbuf, 128), R.RT(pbuf, 128)
    timer = _time_device if xbuf.is_cuda else _time_host
    for j in (1, n // 2):
        g = R.CswapGeom(outer, n, 1, -1, n, j, False)
        cases = {
            "diff": (lambda: R.cswap_diff(x4, g, nb=1), lambda: R.cswap_diff_torch(x4, g, nb=1)),
            "cross": (lambda: R.cswap_cross(s0, s1, x0, x1, g, nb=1),
                      lambda: R.cswap_cross_torch(s0, s1, x0, x1, g, nb=1)),
            "apply": (lambda: R.cswap_apply(x4, p4, g, nb=1),
                      lambda: R.cswap_apply_torch(x4, p4, g, nb=1)),
        }
        for name, (kernel, torch_) in cases.items():
            assert torch.equal(kernel().data, torch_().data)  # bit for bit
            for path, fn in (("kernel", kernel), ("torch", torch_)):
                ms = timer(fn, warmup, runs)
                rec = {"bench": "sort.leaf", "leaf": name, "path": path, "j": j,
                       "shape": [outer, n], "repeat": repeat, "p50_ms": ms,
                       "device": str(device)}
                out.append(rec)
                print(json.dumps(rec), flush=True)
    return out


def programs():
    alice, bob, carole = (pm.host_placement(n) for n in ROLES)
    rep = pm.replicated_placement("rep", players=[alice, bob, carole])
    dt = pm.fixed(24, 40)

    def make(body, shape):
        @pm.computation
        def prog(x: pm.Argument(placement=alice, vtype=pm.TensorType(pm.float64), shape=shape)):
            with alice:
                xf = pm.cast(x, dtype=dt)
            with rep:
                y = body(xf)
            with carole:
                return pm.cast(y, dtype=pm.float64)

        return prog

    rng = np.random.default_rng(0)
    grid = lambda a: np.round(a * 2.0 ** 40) / 2.0 ** 40  # noqa: E731
    xs = grid(rng.uniform(-100, 100, SORT))
    xr = grid(rng.uniform(-100, 100, ROWS))
    xr[:, 0] = rng.permutation(ROWS[0]) - ROWS[0] / 2  # distinct keys
    return {"sort": (make(lambda v: pm.sort(v), SORT), xs, np.sort(xs, axis=-1)),
            "sort_rows": (make(lambda v: pm.sort_rows(v, by=0), ROWS), xr,
                          xr[np.argsort(xr[:, 0])])}


def replay(device, warmup, runs, repeat):
    out = []
    cuda = str(device).startswith("cuda")
    for name, (comp, x, want) in programs().items():
        for leaf_path in ("kernel", "torch"):
            keep, R.CSWAP_KERNEL = R.CSWAP_KERNEL, leaf_path == "kernel"
            try:
                rt = pm.LocalMooseRuntime(ROLES, device=device, use_graphs=cuda)
                got = rt.evaluate_computation(comp, {"x": x})["output_0"]
                assert np.array_equal(got, want)
                ms = _time_host(lambda: rt.evaluate_computation(comp, {"x": x}), warmup, runs)
            finally:
                R.CSWAP_KERNEL = keep
            rec = {"bench": "sort.program", "program": name, "leaf": leaf_path,
                   "mode": "replay" if cuda else "eager", "shape": list(x.shape),
                   "repeat": repeat, "p50_ms": ms, "device": str(device)}
            out.append(rec)
            print(json.dumps(rec), flush=True)
    return out


def nodes(device, warmup, runs):
    """The programs with the three parties as threads on this GPU, whose tapes are composed
    into one hipGraph that reports its nodes."""
    out = []
    for name, (comp, x, want) in programs().items():
        rt = pm.LocalMooseRuntime(ROLES, device_map={r: device for r in ROLES},
                                  use_graphs=True, timeout=120)
        ms = _time_host(lambda: rt.evaluate_computation(comp, {"x": x}), max(warmup, 3), runs)
        # what is timed is the replay, so that is what is checked (docs/NEXT.md: before the
        # tapes are composed, a per-party sign extraction of 65,536 elements on one device
        # goes wrong, for relu as for a sort)
        assert np.array_equal(rt.evaluate_computation(comp, {"x": x})["output_0"], want)
        tapes = [t for _, t in rt._party_tapes.values() if t]
        gn = (tapes[0].graph_nodes or {}) if tapes else {}
        rec = {"bench": "sort.program", "program": name, "mode": "parties_replay", "p50_ms": ms,
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
    ap.add_argument("--part", choices=("all", "leaf", "replay", "nodes"), default="all")
    a = ap.parse_args(argv)

    import torch

    device = a.device or ("cuda:0" if torch.cuda.is_available() else "cpu")
    results = []
    for r in range(a.repeats):
        if a.part in ("all", "leaf"):
            results += leaf(device, a.warmup, a.runs, r)
        if a.part in ("all", "replay"):
            results += replay(device, a.warmup, a.runs, r)
    if a.part in ("all", "nodes") and str(device).startswith("cuda"):
        results += nodes(device, a.warmup, a.runs)
    return results


if __name__ == "__main__":
    main()
