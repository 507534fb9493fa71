"""The native ABI in its three places: the ctypes table of moose_amd/ops/native.py, the built
library, and csrc/moosex.h."""
import os
import re

from moose_amd.ops import native as nat

# entry points that were removed: they come back in none of the three places
RETIRED = ["mx_gemm_ws", "mx_gemm_workspace_bytes"]


def test_every_name_of_the_table_resolves_in_the_library():
    lib = nat.lib()
    missing = [name for name in nat._SIGS if not hasattr(lib, name)]
    assert not missing, missing


def test_retired_entry_points_are_gone_everywhere():
    lib = nat.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "csrc",
                               "moosex.h")).read()
    for name in RETIRED:
        assert name not in nat._SIGS, name
        assert not hasattr(lib, name), name
        assert not re.search(rf"\b{name}\b", header), name
