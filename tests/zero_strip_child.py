"""Child process of tests/test_zero_strip.py: the library reads MOOSEX_ZERO_STRIP and
MOOSEX_CRT_KERNEL once, so a run under another value needs a fresh process.

reveal: one share -> dot -> reveal through the runtime on a seeded session; prints the
        revealed bits' digest and the SessionStats.
kernel: the product from share sources against mx_share3_k + mx_gemm_asym, every owner and
        direction, each side and both (test_zero_strip._Case.check); prints "ok"."""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def reveal():
    import moose_amd as pm

    alice, bob, carole = (pm.host_placement(n) for n in ("alice", "bob", "carole"))
    rep = pm.replicated_placement("rep", players=[alice, bob, carole])
    f64 = pm.TensorType(pm.float64)

    @pm.computation
    def comp(x: pm.Argument(placement=alice, vtype=f64),
             y: pm.Argument(placement=bob, vtype=f64)):
        with alice:
            xf = pm.cast(x, dtype=pm.fixed(14, 23))
        with bob:
            yf = pm.cast(y, dtype=pm.fixed(14, 23))
        with rep:
            z = pm.dot(xf, yf)
        with carole:
            out = pm.cast(z, dtype=pm.float64)
        return out

    rng = np.random.default_rng(5)
    args = {"x": rng.uniform(-1, 1, (256, 256)), "y": rng.uniform(-1, 1, (256, 256))}
    rt = pm.LocalMooseRuntime(["alice", "bob", "carole"], device="cuda:0", seed=21,
                              use_graphs=False, fixedpoint_ring=128)
    out = np.ascontiguousarray(rt.evaluate_computation(comp, args)["output_0"])
    assert np.abs(out - args["x"] @ args["y"]).max() < 1e-4
    st = rt.last_stats.as_dict()
    print(json.dumps({"bits": hashlib.sha256(out.tobytes()).hexdigest(),
                      "stats": {k: st[k] for k in ("rounds", "reshare_bytes", "bytes",
                                                   "messages")}}))


def kernel():
    import test_zero_strip as t

    case = t._Case((256, 256, 256), t.F64)
    for j0 in range(3):
        for d in (1, 2):
            for side in ("x", "y", "xy"):
                case.check(side, j0, d)
    print("ok")


if __name__ == "__main__":
    {"reveal": reveal, "kernel": kernel}[sys.argv[1]]()
