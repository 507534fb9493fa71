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


def _prototypes(text):
    """Names of the mx_* / mxh_* function declarations (ending in ``;``) of a header text."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return sorted(set(re.findall(r"\b(mxh?_\w+)\s*\([^;{}]*\)\s*;", text)))


def test_every_prototype_of_the_headers_resolves_in_the_library():
    lib = nat.lib()
    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "csrc")
    host = _prototypes(open(os.path.join(csrc, "moosex.h")).read())
    common = open(os.path.join(csrc, "ring_common.h")).read()
    block = re.search(r'^extern "C" \{\n(.*?)^\}', common, flags=re.S | re.M)
    assert block, "ring_common.h: no extern \"C\" block"
    dev = _prototypes(block.group(1))
    # the parser sees the headers (91 and 49 prototypes when this was written): a pattern
    # that matched only a few would make the check below vacuous
    assert len(host) >= 80 and "mx_ew_binary" in host and "mx_cswap_apply" in host, len(host)
    assert len(dev) >= 40 and "mxh_ew_binary" in dev and "mxh_gemm" in dev, len(dev)
    assert all(n.startswith("mxh_") for n in dev), dev
    missing = [name for name in host + dev if not hasattr(lib, name)]
    assert not missing, missing


def test_retired_entry_points_are_gone_everywhere():
    lib = nat.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "csrc",
                               "moosex.h")).read()
    for name in RETIRED:
        assert name not in nat._SIGS, name
        assert not hasattr(lib, name), name
        assert not re.search(rf"\b{name}\b", header), name
