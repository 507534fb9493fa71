"""Secure 2-D convolution: the im2col gather alone, and a LeNet-size network.

(a) ``R.im2col`` (the ``k_im2col`` kernel) against the torch composition the primitive would
    otherwise be (zero pad + ``as_strided`` + ``contiguous``, ``R.im2col_torch``) on a stacked
    share buffer of four slots over Z_2^128, 3x3, pad 1: ``[4, 8, 32, 32, 16]`` NHWC and
    ``[4, 8, 16, 32, 32]`` NCHW.  p50 of the timed calls (device events), and the effective
    GB/s = (bytes read + bytes written) / time.
(b) 1x28x28 -> conv 5x5x6 -> ReLU -> avgpool 2 -> conv 5x5x16 -> ReLU -> avgpool 2 ->
    256-120-10 with random weights at fixed(24, 40), batch 1 and 16, on LocalMooseRuntime,
    eager and with hipGraph replay, and with the three parties as threads on the GPU
    (composed replay), which is where the graph's node count comes from.

Everything is measured twice (``--repeats``); one JSON line per measurement, no threshold.

Usage::

    python benchmarks/conv2d.py [--runs 50] [--warmup 5] [--repeats 2] [--device cuda:0]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import moose_amd as pm  # noqa: E402
from moose_amd.models.predictors.conv import ConvNetwork  # noqa: E402
from moose_amd.ops import ring as R  # noqa: E402

ROLES = ["alice", "bob", "carole"]
GATHER = {"NHWC": (4, 8, 32, 32, 16), "NCHW": (4, 8, 16, 32, 32)}
KERNEL, STRIDES, PADS, DIL = (3, 3), (1, 1), (1, 1, 1, 1), (1, 1)


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


def gather(device, warmup, runs, repeat):
    import torch

    out = []
    for fmt, shape in GATHER.items():
        data = torch.randint(-2 ** 62, 2 ** 62, shape + (2,), dtype=torch.int64, device=device)
        a = R.RT(data, 128)
        geom = R.im2col_geometry(shape[1:], KERNEL, STRIDES, PADS, DIL, fmt)
        kern = lambda: R.im2col(a, KERNEL, STRIDES, PADS, DIL, fmt, nb=1)  # noqa: E731
        comp = lambda: R.im2col_torch(a.data, geom, fmt, 1)  # noqa: E731
        assert torch.equal(kern().data, comp())
        timer = _time_device if data.is_cuda else _time_host
        nbytes = 16 * (data.numel() // 2 + kern().numel())
        for name, fn in (("kernel", kern), ("torch", comp)):
            ms = timer(fn, warmup, runs)
            rec = {"bench": "conv2d.gather", "path": name, "format": fmt, "shape": list(shape),
                   "repeat": repeat, "p50_ms": ms, "gbps": nbytes / ms / 1e6,
                   "device": str(device)}
            out.append(rec)
            print(json.dumps(rec), flush=True)
    return out


def lenet(seed=3):
    rng = np.random.default_rng(seed)
    u = lambda *s: rng.uniform(-1, 1, s) / np.sqrt(np.prod(s[1:]))  # noqa: E731
    pool = {"op": "avgpool", "kernel": (2, 2), "strides": (2, 2), "pads": (0, 0, 0, 0)}
    conv = lambda oc, c: {"op": "conv", "w": u(oc, c, 5, 5), "b": u(oc), "strides": (1, 1),  # noqa: E731
                          "pads": (0, 0, 0, 0), "dilations": (1, 1)}
    return ConvNetwork((1, 28, 28), [
        conv(6, 1), {"op": "relu"}, dict(pool), conv(16, 6), {"op": "relu"}, dict(pool),
        {"op": "flatten"}, {"op": "dense", "w": u(256, 120), "b": u(120)}, {"op": "relu"},
        {"op": "dense", "w": u(120, 10), "b": u(10)}])


def network(device, warmup, runs, repeat):
    out = []
    net = lenet()
    comp = net.predictor_factory(pm.fixed(24, 40))
    for batch in (1, 16):
        x = np.random.default_rng(batch).uniform(-1, 1, (batch, 1, 28, 28))
        for mode, graphs in (("eager", False), ("replay", True)):
            if graphs and not str(device).startswith("cuda"):
                continue
            rt = pm.LocalMooseRuntime(ROLES, device=device, use_graphs=graphs)
            ms = _time_host(lambda: rt.evaluate_computation(comp, {"x": x}), warmup, runs)
            rec = {"bench": "conv2d.lenet", "mode": mode, "batch": batch, "repeat": repeat,
                   "p50_ms": ms, "device": str(device)}
            out.append(rec)
            print(json.dumps(rec), flush=True)
        if not str(device).startswith("cuda"):
            continue
        # the graph's kernel count: the stacked runtime's captured graphs expose none, so it
        # is taken from the same network with the three parties as threads on this GPU,
        # whose tapes are composed into one hipGraph that reports its nodes
        rt = pm.LocalMooseRuntime(ROLES, device_map={r: device for r in ROLES},
                                  use_graphs=True, timeout=60)
        ms = _time_host(lambda: rt.evaluate_computation(comp, {"x": x}), warmup, runs)
        tapes = [t for _, t in rt._party_tapes.values() if t]
        gn = (tapes[0].graph_nodes or {}) if tapes else {}
        rec = {"bench": "conv2d.lenet", "mode": "parties_replay", "batch": batch,
               "repeat": repeat, "p50_ms": ms, "device": str(device), "replayed": bool(tapes),
               "nodes": gn.get("nodes"), "party_batched": gn.get("party_batched")}
        out.append(rec)
        print(json.dumps(rec), flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--device", default=None)
    a = ap.parse_args(argv)

    import torch

    device = a.device or ("cuda:0" if torch.cuda.is_available() else "cpu")
    results = []
    for r in range(a.repeats):
        results += gather(device, a.warmup, a.runs, r)
        results += network(device, a.warmup, a.runs, r)
    return results


if __name__ == "__main__":
    main()
