"""QPN_OPT_CRASH_CACHE in the ABI (no compute calls): the header defines the option, the Python mirror carries the same value, the
Julia shim names it too, and qpn_nodes_info still takes the four int32_t it took (the cache state rides in spare bits of info[2])."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "qpn_hip.h")).read()


def test_header_defines_the_option_and_the_mirrors_agree():
    from qpn_amd import _lib
    m = re.search(r"^#define\s+QPN_OPT_CRASH_CACHE\s+(\d+)\s*$", _header(), re.M)
    assert m, "include/qpn_hip.h does not define QPN_OPT_CRASH_CACHE"
    value = int(m.group(1))
    assert _lib.OPT_CRASH_CACHE == value
    others = {int(v) for v in re.findall(r"^#define\s+QPN_OPT_(?!CRASH_CACHE)\w+\s+(\d+)\s*$", _header(), re.M)}
    assert value not in others, "option numbers must be distinct"
    jl = open(os.path.join(ROOT, "julia", "QPNHip.jl")).read()
    mj = re.search(r"const\s+QPN_OPT_CRASH_CACHE\s*=\s*Int32\((\d+)\)", jl)
    assert mj and int(mj.group(1)) == value


def test_nodes_info_keeps_its_signature():
    assert re.search(r"int\s+qpn_nodes_info\s*\(\s*qpn_ctx\s*\*\s*ctx\s*,\s*qpn_nodes\s*\*\s*nodes\s*,\s*int32_t\s+info\[4\]\s*\)\s*;",
                     _header())
    src = open(os.path.join(ROOT, "quadraticprogramnetworks.jl_amd", "csrc", "qpn_capi_nodes.hip")).read()
    assert re.search(r"int\s+qpn_nodes_info\s*\(\s*qpn_ctx\s*\*\s*ctx\s*,\s*qpn_nodes\s*\*\s*h\s*,\s*int32_t\s+info\[4\]\s*\)", src)


def test_library_exports_what_the_option_needs():
    from qpn_amd import _lib
    lib = _lib.load_library()
    assert hasattr(lib, "qpn_ctx_set_option") and hasattr(lib, "qpn_nodes_info")
