"""Secure image resize: the stencil kernel against the torch composition, and a small decoder.

(a) ``R.resize`` (the ``k_resize2d`` kernel) on a stacked share buffer of four slots over
    Z_2^128 against ``R.resize_torch`` (``index_select`` + integer multiply + add on 32-bit
    limbs, one carry pass) in the same process: ``[4, 8, 32, 32, 16]`` NHWC and ``[4, 8, 16,
    32, 32]`` NCHW to 64 x 64, bilinear ``half_pixel`` and nearest.  ``R.im2col`` (3x3, pad 1)
    of the same image is timed alongside.  p50 of the timed calls (device events), and the
    effective GB/s = (bytes read + bytes written) / time, each input pixel counted once.
(b) ``benchmarks/conv_transpose.py``'s decoder with every ConvTranspose replaced by a 2x
    bilinear ``pm.resize2d`` + 3x3 ``pm.conv2d``: latent 32 -> dense 392 -> 7x7x8 -> resize
    14x14 -> conv (8 -> 4) -> ReLU -> resize 28x28 -> conv (4 -> 1), random weights at
    fixed(24, 40), batch 1 and 16, on LocalMooseRuntime, eager and with hipGraph replay.

Everything is measured twice (``--repeats``); one JSON line per measurement, no threshold.

Usage::

    python benchmarks/resize.py [--runs 50] [--warmup 5] [--repeats 2] [--device cuda:0]
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
SIZES = (64, 64)
MODES = {"bilinear": dict(mode="linear", coordinate_transformation_mode="half_pixel",
                          weight_bits=(2, 2)),
         "nearest": dict(mode="nearest", coordinate_transformation_mode="asymmetric",
                         nearest_mode="floor")}


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


def stencil(device, warmup, runs, repeat):
    import torch

    out = []
    for fmt, shape in IMAGE.items():
        img = R.RT(torch.randint(-2 ** 62, 2 ** 62, shape + (2,), dtype=torch.int64,
                                 device=device), 128)
        timer = _time_device if img.data.is_cuda else _time_host
        gather = lambda: R.im2col(img, (3, 3), (1, 1), (1, 1, 1, 1), (1, 1), fmt, nb=1)  # noqa: E731
        paths = []
        for name, attrs in MODES.items():
            geom = R.resize_geometry(shape[1:], SIZES, attrs["mode"],
                                     attrs["coordinate_transformation_mode"],
                                     attrs.get("nearest_mode", "round_prefer_floor"), (),
                                     attrs.get("weight_bits", (0, 0)), fmt)
            kernel = lambda a=attrs: R.resize(img, SIZES, data_format=fmt, nb=1, **a)  # noqa: E731
            torch_ = lambda a=attrs, g=geom: R.resize_torch(  # noqa: E731
                img.data, g, a["mode"], a["coordinate_transformation_mode"],
                a.get("nearest_mode", "round_prefer_floor"), fmt, 1, 128)
            got = kernel()
            # the composition and, on one slot, the CPU twin: bit for bit
            assert torch.equal(got.data, torch_())
            want = R.resize(R.RT(img.data[1].cpu(), 128), SIZES, data_format=fmt, **attrs)
            assert torch.equal(got.data[1].cpu(), want.data)
            nbytes = 16 * (img.data.numel() // 2 + got.data.numel() // 2)
            paths += [(name, "kernel", kernel, nbytes), (name, "torch", torch_, nbytes)]
        cols = gather()
        paths.append(("im2col", "kernel", gather,
                      16 * (img.data.numel() // 2 + cols.data.numel() // 2)))
        for mode, path, fn, nbytes in paths:
            ms = timer(fn, warmup, runs)
            rec = {"bench": "resize.stencil", "mode": mode, "path": path, "format": fmt,
                   "image": list(shape), "sizes": list(SIZES), "repeat": repeat, "p50_ms": ms,
                   "gbps": nbytes / ms / 1e6, "device": str(device)}
            out.append(rec)
            print(json.dumps(rec), flush=True)
    return out


def decoder(seed=3):
    rng = np.random.default_rng(seed)
    u = lambda *s: rng.uniform(-1, 1, s) / np.sqrt(np.prod(s[1:]))  # noqa: E731
    wd, bd = u(32, 392), u(392)
    w1, b1, w2, b2 = u(4, 8, 3, 3), u(4), u(1, 4, 3, 3), u(1)
    alice, bob, carole = (pm.host_placement(n) for n in ROLES)
    rep = pm.replicated_placement("rep", players=[alice, bob, carole])
    mir = pm.mirrored_placement("mir", players=[alice, bob, carole])
    dt = pm.fixed(24, 40)
    conv = dict(pads=(1, 1, 1, 1), data_format="NHWC")
    up = dict(scales=(2.0, 2.0), mode="linear", data_format="NHWC")

    @pm.computation
    def decode(z: pm.Argument(placement=alice, vtype=pm.TensorType(pm.float64))):
        with alice:
            zf = pm.cast(z, dtype=dt)
        with mir:
            c = [pm.cast(pm.constant(v), dtype=dt) for v in (wd, bd, w1, b1, w2, b2)]
        with rep:
            h = pm.relu(pm.add(pm.dot(zf, c[0]), c[1]))
            h = pm.reshape(h, [-1, 7, 7, 8])
            h = pm.resize2d(h, input_shape=(None, 7, 7, 8), **up)
            h = pm.relu(pm.conv2d(h, c[2], c[3], weight_shape=w1.shape, **conv))
            h = pm.resize2d(h, **up)
            y = pm.conv2d(h, c[4], c[5], weight_shape=w2.shape, **conv)
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
            rec = {"bench": "resize.decoder", "mode": mode, "batch": batch,
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
        results += stencil(device, a.warmup, a.runs, r)
        results += network(device, a.warmup, a.runs, r)
    return results


if __name__ == "__main__":
    main()
