"""Child process of tests/test_crt_variants.py: the library reads MOOSEX_CRT_RECON once, so a
run under another value needs a fresh process.  Under the environment it is started with it
checks, for both rings, the CRT products (test_crt_variants.Case.check) and an accumulate into
a non-zero C against the limb GEMM, and prints one JSON line: whether they held, the answer
of mx_crt_defer_bytes and the code of mx_gemm_asym with a ``residues`` buffer."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    import torch

    import test_crt_variants as t
    from moose_amd.ops import native as nat
    from moose_amd.ops import ring as R

    out = {"defer_bytes": {}, "asym_residues_rc": {}}
    for bits in (64, 128):
        c = t.case(bits)
        c.check()
        # C += x0.(y0 + y1) + x1.y0 on a non-zero C
        base = t.rand_rt((3, t.M, t.N), bits, 230)
        acc = R.RT(base.data.clone(), bits)
        with t._crt(1):
            R._gemm_call(bits, 3, t.M, t.N, t.K, c.x0.data, c.x1.data, c.ys[0].data, c.ys[1].data,
                         1, acc.data, accumulate=1)
        assert torch.equal(acc.data, R.binary("add", base, c.cross).data), bits
        words = bits // 64
        nbytes = nat.lib().mx_crt_defer_bytes(words, t.M, t.N, t.K)
        out["defer_bytes"][str(bits)] = nbytes
        res = torch.empty(max(nbytes, 16), dtype=torch.int8, device="cuda")
        rc = nat.lib().mx_gemm_asym(words, t.M, t.N, t.K, nat.ptr(c.x0.data), None,
                                    nat.ptr(c.y0.data), None, 1, None, nat.stream_of(res),
                                    nat.ptr(res))
        out["asym_residues_rc"][str(bits)] = rc
        if rc == 0:  # the deferred product, reconstructed, is the product
            got = R.empty((3, t.M, t.N), bits, res.device)
            nat.check(nat.lib().mx_crt_recon(words, t.M, t.N, t.K, nat.ptr(res),
                                             nat.ptr(got.data), nat.stream_of(res)), "crt_recon")
            assert torch.equal(got.data, c.asym.data), bits
    torch.cuda.synchronize()
    out["products"] = "ok"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
