"""Child process of tests/test_gemm_exact.py: the library reads MOOSEX_GEMM_V and
MOOSEX_GEMM_SPLIT once, so the v1 limb kernels need a fresh process.  Under the environment it
is started with it runs test_gemm_exact.child_checks (every product against the integer
oracle), ends at the first failure, and prints one JSON line."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    import test_gemm_exact as t

    n = t.child_checks()
    env = {k: os.environ[k] for k in ("MOOSEX_GEMM_V", "MOOSEX_GEMM_SPLIT") if k in os.environ}
    print(json.dumps({"ok": True, "cases": n, "env": env}))


if __name__ == "__main__":
    main()
