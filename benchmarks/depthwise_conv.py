"""Secure depthwise convolution: the direct ring kernel against the block-diagonal workaround.

NHWC ``[8, 32, 32, 64]``, 3x3, pad 1, ``mult = 1``, at Z_2^128 / fixed(24, 40), secret image
and secret weight, on LocalMooseRuntime with hipGraph replay on a device:

(1) ``pm.depthwise_conv2d``: the ``DepthwiseConv`` operator (``k_dwconv`` + the dot tail);
(2) the same convolution as ``pm.conv2d`` with the weight expanded to block-diagonal
    ``[64, 64, 3, 3]`` (im2col + the fixed-point dot), which is what a depthwise convolution
    had to be before the operator existed -- that code path is unchanged by it;
(3) the kernel alone: ``R.dwconv_cross`` on the two views of a four-slot share-pair buffer,
    as effective GB/s = (distinct bytes read + bytes written) / time.

(1) and (2) alternate, ``--repeats`` times; p50 of ``--runs`` timed calls each; one JSON line
per measurement, no threshold.

Usage::

    python benchmarks/depthwise_conv.py [--runs 50] [--warmup 5] [--repeats 2] [--device cuda:0]
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
SHAPE, C = (8, 32, 32, 64), 64
PADS = (1, 1, 1, 1)
DT = pm.fixed(24, 40)


def _p50(fn, warmup, runs, sync=None):
    for _ in range(warmup):
        fn()
    lat = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        if sync is not None:
            sync()
        lat.append((time.perf_counter() - t0) * 1e3)
    lat.sort()
    return lat[len(lat) // 2]


def _program(w, depthwise):
    alice, bob, carole = (pm.host_placement(n) for n in ROLES)
    rep = pm.replicated_placement("rep", players=[alice, bob, carole])

    @pm.computation
    def prog(x: pm.Argument(placement=alice, vtype=pm.TensorType(pm.float64), shape=SHAPE)):
        with alice:
            xf = pm.cast(x, dtype=DT)
        with bob:
            wf = pm.cast(pm.constant(w), dtype=DT)
        with rep:
            if depthwise:
                y = pm.depthwise_conv2d(xf, wf, pads=PADS, data_format="NHWC")
            else:
                y = pm.conv2d(xf, wf, pads=PADS, data_format="NHWC")
        with carole:
            return pm.cast(y, dtype=pm.float64)

    return prog


def programs(seed=3):
    rng = np.random.default_rng(seed)
    w = rng.uniform(-1, 1, (C, 1, 3, 3)) / 3
    dense = np.zeros((C, C, 3, 3))
    dense[np.arange(C), np.arange(C)] = w[:, 0]
    x = rng.uniform(-1, 1, SHAPE)
    return x, _program(w, True), _program(dense, False)


def end_to_end(device, warmup, runs, repeat, state):
    out = []
    if not state:
        x, dw, bd = programs()
        graphs = str(device).startswith("cuda")
        state.update(x=x, paths=[
            ("depthwise", dw, pm.LocalMooseRuntime(ROLES, device=device, use_graphs=graphs)),
            ("block_diagonal", bd, pm.LocalMooseRuntime(ROLES, device=device,
                                                        use_graphs=graphs))])
        a, b = (rt.evaluate_computation(comp, {"x": x})["output_0"]
                for _, comp, rt in state["paths"])
        state["max_abs_diff"] = float(np.abs(a - b).max())
    for name, comp, rt in state["paths"]:
        ms = _p50(lambda: rt.evaluate_computation(comp, {"x": state["x"]}), warmup, runs)
        rec = {"bench": "depthwise_conv.e2e", "path": name, "shape": list(SHAPE),
               "repeat": repeat, "p50_ms": ms, "device": str(device),
               "max_abs_diff_between_paths": state["max_abs_diff"]}
        out.append(rec)
        print(json.dumps(rec), flush=True)
    return out


def kernel(device, warmup, runs, repeat):
    import torch

    xb = torch.randint(-2 ** 62, 2 ** 62, (4,) + SHAPE + (2,), dtype=torch.int64, device=device)
    wb = torch.randint(-2 ** 62, 2 ** 62, (4, C, 1, 3, 3, 2), dtype=torch.int64, device=device)
    x0, x1, w0, w1 = (R.RT(t, 128) for t in (xb[0:3], xb[1:4], wb[0:3], wb[1:4]))
    fn = lambda: R.dwconv_cross(x0, x1, w0, w1, (1, 1), PADS, (1, 1), "NHWC", nb=1)  # noqa: E731
    out = fn()
    nbytes = 8 * (xb.numel() + wb.numel() + out.data.numel())
    if xb.is_cuda:
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
        ms = lat[len(lat) // 2]
    else:
        ms = _p50(fn, warmup, runs)
    rec = {"bench": "depthwise_conv.kernel", "mode": "cross", "slots": 3, "shape": list(SHAPE),
           "repeat": repeat, "p50_ms": ms, "gbps": nbytes / ms / 1e6, "device": str(device)}
    print(json.dumps(rec), flush=True)
    return [rec]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--device", default=None)
    a = ap.parse_args(argv)

    import torch

    device = a.device or ("cuda:0" if torch.cuda.is_available() else "cpu")
    results, state = [], {}
    for r in range(a.repeats):
        results += end_to_end(device, a.warmup, a.runs, r, state)
        results += kernel(device, a.warmup, a.runs, r)
    return results


if __name__ == "__main__":
    main()
