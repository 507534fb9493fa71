"""Mixed-ring logistic-regression inference against the all-Z_2^128 program.

The shape of the LR inference benchmark (200 rows, 10 features; ``x`` secret-shared from
alice, the weights from bob, the probabilities revealed to carole), in two forms:

* ``all128``: every step over Z_2^128 at ``fixed(24, 40)``;
* ``mixed``: the dot over Z_2^64 at ``fixed(8, 23, ring=64)``, the product widened to
  ``fixed(24, 40, ring=128)`` by the exact ring extension, the sigmoid over Z_2^128.

Each runs on (a) the stacked session and (b) the three parties as threads on one GPU with
``use_graphs=True`` (their tapes composed into one hipGraph), (b) once with the per-party
ring-extension kernels (``replicated.PARTY_RING_EXTEND``) and once with the composed
protocol.  One process, warm-up evaluations first, medians of the timed ones; for (b) the
composed graph's node counts.  One JSON line per measurement; no pass/fail threshold.

Usage::

    python benchmarks/mixed_ring_lr.py [--runs 50] [--warmup 5] [--device cuda:0]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import moose_amd as pm  # noqa: E402
from moose_amd.protocols import replicated  # noqa: E402

ROLES = ["alice", "bob", "carole"]
NARROW = pm.fixed(8, 23, ring=64)
WIDE = pm.fixed(24, 40, ring=128)


def build(mixed: bool):
    alice, bob, carole = (pm.host_placement(n) for n in ROLES)
    rep = pm.replicated_placement(name="rep", players=[alice, bob, carole])
    arg = lambda p: pm.Argument(placement=p, vtype=pm.TensorType(pm.float64))  # noqa: E731

    @pm.computation
    def comp(x: arg(alice), w: arg(bob)):
        with alice:
            xf = pm.cast(x, dtype=NARROW if mixed else WIDE)
        with bob:
            wf = pm.cast(w, dtype=NARROW if mixed else WIDE)
        with rep:
            z = pm.dot(xf, wf)
            if mixed:
                z = pm.cast(z, dtype=WIDE)
            p = pm.sigmoid(z)
        with carole:
            return pm.cast(p, dtype=pm.float64)

    return comp


def measure(rt, comp, args, warmup, runs):
    for _ in range(warmup):
        out = rt.evaluate_computation(comp, args)
    lat = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = rt.evaluate_computation(comp, args)  # synchronises the device
        lat.append((time.perf_counter() - t0) * 1e3)
    lat.sort()
    return np.asarray(out["output_0"]), {"p50_ms": lat[len(lat) // 2],
                                         "p90_ms": lat[int(0.9 * (len(lat) - 1))]}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--device", default=None)
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--features", type=int, default=10)
    a = ap.parse_args(argv)

    import torch

    device = a.device or ("cuda:0" if torch.cuda.is_available() else "cpu")
    rng = np.random.default_rng(5)
    args = {"x": rng.normal(0, 1, (a.rows, a.features)),
            "w": rng.normal(0, 0.5, (a.features, 1))}
    want = 1 / (1 + np.exp(-(args["x"] @ args["w"])))
    results = []
    for form in ("all128", "mixed"):
        comp = build(form == "mixed")
        cases = [("stacked", True, {"device": device, "use_graphs": True})]
        for on in ((True, False) if form == "mixed" else (True,)):
            cases.append(("parties", on, {"device_map": {r: device for r in ROLES},
                                          "use_graphs": True, "timeout": 60}))
        for layout, on, flags in cases:
            replicated.PARTY_RING_EXTEND = on
            try:
                rt = pm.LocalMooseRuntime(ROLES, **flags)
                out, rec = measure(rt, comp, args, a.warmup, a.runs)
            finally:
                replicated.PARTY_RING_EXTEND = True
            rec.update(bench="mixed_ring_lr", form=form, layout=layout, device=device,
                       rows=a.rows, features=a.features, runs=a.runs,
                       max_abs_err=float(np.abs(out - want).max()))
            if layout == "parties":
                rec["party_ring_extend"] = on
                tapes = [t for _, t in rt._party_tapes.values() if t]
                rec["replayed"] = bool(tapes)
                rec["rounds"] = rt.last_stats.rounds
                if tapes:
                    rec["replay_form"] = tapes[0].replay_form
                    gn = tapes[0].graph_nodes or {}
                    rec["nodes"] = gn.get("nodes")
                    rec["party_batched"] = gn.get("party_batched")
            results.append(rec)
            print(json.dumps(rec), flush=True)
    return results


if __name__ == "__main__":
    main()
