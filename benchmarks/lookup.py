"""Secure demultiplexer: the outer-product kernel against its torch composition, and
``rep.demux`` with either as the leaf.

(a) ``R.outer_cross`` (the ``k_outer_cross`` kernel) against ``R.outer_cross_torch`` in the same
    process, in cross mode on the share vectors of a four-slot Z_2^128 buffer, with L and H the
    paired groups of one state read in place, at ``(groups, rows, A, B) = (1, 4096, 32, 32)`` and
    ``(4, 65536, 4, 4)``.  p50 of the timed calls (device events).
(b) eager ``rep.demux`` of 4096 secret 10-bit indices into 1024 one-hot columns over Z_2^128 on a
    stacked session, with the kernel and with the composition as the leaf.
(c) replayed ``pm.lookup`` of 4096 indices into a secret ``[1024, 16]`` table at fixed(24, 40), and
    replayed ``pm.bincount`` with weights ``[65536, 3]`` over 16 categories against
    ``pm.group_by_sum(shuffle=False)`` of the same ``[65536, 4]`` table, on LocalMooseRuntime.

Everything is measured twice (``--repeats``); one JSON line per measurement, no threshold.

Usage::

    python benchmarks/lookup.py [--runs 50] [--warmup 5] [--repeats 2] [--device cuda:0]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import moose_amd as pm  # noqa: E402
from moose_amd.ops import ring as R  # noqa: E402

ROLES = ["alice", "bob", "carole"]

SHAPES = ((1, 4096, 32, 32), (4, 65536, 4, 4))
DEMUX = (4096, 1024)  # rows, outputs


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
    for groups, rows, A, B in SHAPES:
        assert A == B  # the pairs of one state
        xbuf = torch.randint(-2 ** 62, 2 ** 62, (4, 2 * groups, rows, A, 2), dtype=torch.int64,
                             device=device)
        (l0, h0), (l1, h1) = (R.outer_pairs(R.RT(xbuf[q:q + 3], 128), nb=1) for q in (0, 1))
        g = R.OuterGeom(groups, rows, A, B, A * B)
        timer = _time_device if xbuf.is_cuda else _time_host
        kernel = lambda: R.outer_cross(l0, l1, h0, h1, g, nb=1)  # noqa: E731
        torch_ = lambda: R.outer_cross_torch(l0, l1, h0, h1, g, nb=1)  # noqa: E731
        assert torch.equal(kernel().data, torch_().data)  # bit for bit
        for path, fn in (("kernel", kernel), ("torch", torch_)):
            ms = timer(fn, warmup, runs)
            rec = {"bench": "lookup.leaf", "leaf": "outer_cross", "path": path,
                   "shape": [groups, rows, A, B], "repeat": repeat, "p50_ms": ms,
                   "device": str(device)}
            out.append(rec)
            print(json.dumps(rec), flush=True)
    return out


def protocol(device, warmup, runs, repeat):
    import torch

    from moose_amd.ir.computation import ReplicatedPlacement
    from moose_amd.protocols import replicated as rep
    from moose_amd.runtime.session import HV
    from moose_amd.runtime.session import StackedSession

    out = []
    rows, n = DEMUX
    w = rep.demux_width(n)
    plc = ReplicatedPlacement(("a", "b", "c"))
    idx = torch.randint(0, n, (rows,), dtype=torch.int64)
    bits = torch.stack([(idx >> t) & 1 for t in range(w)])
    words = torch.stack([bits, torch.zeros_like(bits)], dim=-1).to(device)
    first = None
    for path in ("kernel", "torch"):
        keep = R.OUTER_KERNEL
        R.OUTER_KERNEL = path == "kernel"
        try:
            sess = StackedSession(device, seed=5)
            planes = rep.share(sess, plc, HV("a", R.RT(words, 128)))
            got = rep.reveal(sess, rep.demux(sess, planes, n), "c").v.data.cpu()
            assert torch.equal(got[..., 0], torch.nn.functional.one_hot(idx, n)) \
                and not got[..., 1].any()
            first = got if first is None else first
            assert torch.equal(got, first)
            timer = _time_device if words.is_cuda else _time_host
            ms = timer(lambda: rep.demux(sess, planes, n), warmup, runs)
        finally:
            R.OUTER_KERNEL = keep
        rec = {"bench": "lookup.demux", "leaf": path, "mode": "eager", "shape": [rows, n],
               "repeat": repeat, "p50_ms": ms, "device": str(device)}
        out.append(rec)
        print(json.dumps(rec), flush=True)
    return out


def programs():
    alice, bob, carole = (pm.host_placement(n) for n in ROLES)
    rep = pm.replicated_placement("rep", players=[alice, bob, carole])
    dt = pm.fixed(24, 40)
    rng = np.random.default_rng(0)
    table = rng.integers(-16 * 256, 16 * 256, size=(1024, 16)) / 256.0
    index = rng.integers(0, 1024, size=(4096,)).astype(np.float64)
    rows = rng.integers(-16 * 256, 16 * 256, size=(65536, 4)) / 256.0
    rows[:, 0] = rng.integers(0, 16, size=65536)

    def arg(a, who):
        return pm.Argument(placement=who, vtype=pm.TensorType(pm.float64), shape=a.shape)

    @pm.computation
    def lookup(t: arg(table, alice), i: arg(index, bob)):
        with alice:
            tf = pm.cast(t, dtype=dt)
        with bob:
            x = pm.cast(i, dtype=dt)
        with rep:
            y = pm.lookup(tf, x)
        with carole:
            return pm.cast(y, dtype=pm.float64)

    def grouped(body):
        @pm.computation
        def prog(t: arg(rows, alice)):
            with alice:
                tf = pm.cast(t, dtype=dt)
            with rep:
                y = body(tf)
            with carole:
                return pm.cast(y, dtype=pm.float64)

        return prog

    def by_bincount(tf):
        n = rows.shape[0]
        key = pm.squeeze(pm.strided_slice(tf, [slice(0, n), slice(0, 1)]), axis=1)
        return pm.bincount(key, 16, weights=pm.strided_slice(tf, [slice(0, n), slice(1, 4)]))

    sums = np.eye(16)[rows[:, 0].astype(int)].T @ rows[:, 1:]

    def check_groups(got):
        valid = got[got[:, -1] == 1.0]
        assert np.array_equal(valid[:, 1:4], sums)

    return {"lookup": (lookup, {"t": table, "i": index},
                       lambda got: np.array_equal(got, table[index.astype(int)])),
            "bincount": (grouped(by_bincount), {"t": rows},
                         lambda got: np.array_equal(got, sums)),
            "group_by_sum": (grouped(lambda tf: pm.group_by_sum(tf, by=0, shuffle=False)),
                             {"t": rows}, lambda got: check_groups(got) is None)}


def program(device, warmup, runs, repeat):
    out = []
    cuda = str(device).startswith("cuda")
    for name, (comp, args, ok) in programs().items():
        rt = pm.LocalMooseRuntime(ROLES, device=device, use_graphs=cuda)
        assert ok(rt.evaluate_computation(comp, args)["output_0"]), name  # exact
        ms = _time_host(lambda: rt.evaluate_computation(comp, args), warmup, runs)
        rec = {"bench": "lookup.program", "program": name,
               "mode": "replay" if cuda else "eager", "repeat": repeat, "p50_ms": ms,
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
    ap.add_argument("--part", choices=("all", "leaf", "protocol", "program"), default="all")
    a = ap.parse_args(argv)

    import torch

    device = a.device or ("cuda:0" if torch.cuda.is_available() else "cpu")
    results = []
    for r in range(a.repeats):
        if a.part in ("all", "leaf"):
            results += leaf(device, a.warmup, a.runs, r)
        if a.part in ("all", "protocol"):
            results += protocol(device, a.warmup, a.runs, r)
        if a.part in ("all", "program"):
            results += program(device, a.warmup, a.runs, r)
    return results


if __name__ == "__main__":
    main()
