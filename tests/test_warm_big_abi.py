"""QPN_OPT_WARM_BIG is one value in the header, the ctypes binding and the Julia shim, behind QPN_OPT_CRASH_CACHE_BIG, and the ABI
version stays what it was."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_one_value_in_every_binding():
    from qpn_amd import _lib
    header = open(os.path.join(ROOT, "include", "qpn_hip.h")).read()
    julia = open(os.path.join(ROOT, "julia", "QPNHip.jl")).read()
    opts = dict(re.findall(r"^#define (QPN_OPT_\w+) (\d+)", header, flags=re.M))
    assert opts["QPN_OPT_WARM_BIG"] == "7" and opts["QPN_OPT_CRASH_CACHE_BIG"] == "6"
    assert sorted(int(v) for v in opts.values()) == list(range(1, 8))           # (99 stays the unknown option of the tests)
    assert re.search(r"^#define QPN_ABI_VERSION 1\b", header, flags=re.M)
    assert _lib.OPT_WARM_BIG == 7
    assert re.search(r"^const QPN_OPT_WARM_BIG = Int32\(7\)", julia, flags=re.M)
    # the header's comment of the options names it
    assert re.search(r"^ \*   QPN_OPT_WARM_BIG ", header, flags=re.M)
