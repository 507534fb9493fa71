"""Secure transposed 2-D convolution: the col2im sum alone, and a small decoder.

(a) ``R.col2im`` (the ``k_col2im`` kernel) on a stacked share buffer of four slots over
    Z_2^128, the mirror image of ``benchmarks/conv2d.py``'s gather: the patch matrix of a
    ``[4, 8, 32, 32, 16]`` NHWC (``[4, 8, 16, 32, 32]`` NCHW) image under 3x3, pad 1, summed
    back into that image.  ``R.im2col`` of the same geometry is timed in the same process: it
    moves the same bytes in the opposite direction.  p50 of the timed calls (device events),
    and the effective GB/s = (bytes read + bytes written) / time.
(b) latent 32 -> dense 392 -> reshape 7x7x8 -> ConvTranspose 4x4 stride 2 pad 1 (8 -> 4,
    14x14) -> ReLU -> ConvTranspose 4x4 stride 2 pad 1 (4 -> 1, 28x28) with
    ``pm.conv_transpose2d`` and random weights at fixed(24, 40), batch 1 and 16, on
    LocalMooseRuntime, eager and with hipGraph replay.

Everything is measured twice (``--repeats``); one JSON line per measurement, no threshold.

Usage::

    python benchmarks/conv_transpose.py [--runs 50] [--warmup 5] [--repeats 2] [--device cuda:0]
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
IMAGE = {"NHWC": (4, 8, 32, 32, 16), "NCHW": (4, 8, 16, 32, 32)}
CHW = (16, 32, 32)
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


def scatter_sum(device, warmup, runs, repeat):
    import torch

    out = []
    for fmt, shape in IMAGE.items():
        img = R.RT(torch.randint(-2 ** 62, 2 ** 62, shape + (2,), dtype=torch.int64,
                                 device=device), 128)
        gather = lambda: R.im2col(img, KERNEL, STRIDES, PADS, DIL, fmt, nb=1)  # noqa: E731
        cols = gather()
        summed = lambda: R.col2im(cols, CHW, KERNEL, STRIDES, PADS, DIL, fmt, nb=1)  # noqa: E731
        # one slot against the CPU twin, bit for bit
        want = R.col2im(R.RT(cols.data[1].cpu(), 128), CHW, KERNEL, STRIDES, PADS, DIL, fmt)
        assert torch.equal(summed().data[1].cpu(), want.data)
        timer = _time_device if img.data.is_cuda else _time_host
        nbytes = 16 * (img.data.numel() // 2 + cols.data.numel() // 2)
        for name, fn in (("col2im", summed), ("im2col", gather)):
            ms = timer(fn, warmup, runs)
            rec = {"bench": "conv_transpose.col2im", "path": name, "format": fmt,
                   "image": list(shape), "repeat": repeat, "p50_ms": ms,
                   "gbps": nbytes / ms / 1e6, "device": str(device)}
            out.append(rec)
            print(json.dumps(rec), flush=True)
    return out


def decoder(seed=3):
    rng = np.random.default_rng(seed)
    u = lambda *s: rng.uniform(-1, 1, s) / np.sqrt(np.prod(s[1:]))  # noqa: E731
    wd, bd = u(32, 392), u(392)
    w1, b1, w2, b2 = u(8, 4, 4, 4), u(4), u(4, 1, 4, 4), u(1)
    alice, bob, carole = (pm.host_placement(n) for n in ROLES)
    rep = pm.replicated_placement("rep", players=[alice, bob, carole])
    mir = pm.mirrored_placement("mir", players=[alice, bob, carole])
    dt = pm.fixed(24, 40)
    geom = dict(strides=(2, 2), pads=(1, 1, 1, 1), data_format="NHWC")

    @pm.computation
    def decode(z: pm.Argument(placement=alice, vtype=pm.TensorType(pm.float64))):
        with alice:
            zf = pm.cast(z, dtype=dt)
        with mir:
            c = [pm.cast(pm.constant(v), dtype=dt) for v in (wd, bd, w1, b1, w2, b2)]
        with rep:
            h = pm.relu(pm.add(pm.dot(zf, c[0]), c[1]))
            h = pm.reshape(h, [-1, 7, 7, 8])
            h = pm.relu(pm.conv_transpose2d(h, c[2], c[3], input_shape=(None, 7, 7, 8), **geom))
            y = pm.conv_transpose2d(h, c[4], c[5], **geom)
        with carole:
            return pm.cast(y, dtype=pm.float64)

    return decode


def network(device, warmup, runs, repeat):
    out = []
    comp = decoder()
    for batch in (1, 16):
        z = np.random.default_rng(batch).uniform(-1, 1, (batch, 32))
        for mode, graphs in (("eager", False), ("replay", True)):
            if graphs and not str(device).startswith("cuda"):
                continue
            rt = pm.LocalMooseRuntime(ROLES, device=device, use_graphs=graphs)
            got = rt.evaluate_computation(comp, {"z": z})["output_0"]
            assert got.shape == (batch, 28, 28, 1)
            ms = _time_host(lambda: rt.evaluate_computation(comp, {"z": z}), warmup, runs)
            rec = {"bench": "conv_transpose.decoder", "mode": mode, "batch": batch,
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
    a = ap.parse_args(argv)

    import torch

    device = a.device or ("cuda:0" if torch.cuda.is_available() else "cpu")
    results = []
    for r in range(a.repeats):
        results += scatter_sum(device, a.warmup, a.runs, r)
        results += network(device, a.warmup, a.runs, r)
    return results


if __name__ == "__main__":
    main()
