"""QPN_OPT_CRASH_CACHE_BIG in the three places that name it: the C header defines it with a value no other QPN_OPT_* has, the
Python mirror and the Julia shim carry the same value; QPN_OPT_CRASH_CACHE keeps its own; the ABI version stays 1."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _header_options():
    opts = {}
    for name, value in re.findall(r"^#define\s+(QPN_OPT_\w+)\s+(-?\d+)\s*$", _read("include", "qpn_hip.h"), re.M):
        assert name not in opts, name
        opts[name] = int(value)
    return opts


def test_header_defines_the_option_with_a_value_of_its_own():
    opts = _header_options()
    assert "QPN_OPT_CRASH_CACHE_BIG" in opts
    assert opts["QPN_OPT_CRASH_CACHE_BIG"] == 6 and opts["QPN_OPT_CRASH_CACHE"] == 4
    assert len(set(opts.values())) == len(opts), opts
    assert re.search(r"^#define\s+QPN_ABI_VERSION\s+1\s*$", _read("include", "qpn_hip.h"), re.M)


def test_python_and_julia_mirror_the_header():
    opts = _header_options()
    lib = _read("quadraticprogramnetworks.jl_amd", "_lib.py")
    jl = _read("julia", "QPNHip.jl")
    for name, value in opts.items():
        py = re.search(rf"^{name[4:]}\s*=\s*(-?\d+)", lib, re.M)
        assert py and int(py.group(1)) == value, name
        ju = re.search(rf"^const {name}\s*=\s*Int32\((-?\d+)\)", jl, re.M)
        assert ju and int(ju.group(1)) == value, name
    # the shim says what the option does, as it does for QPN_OPT_CRASH_CACHE
    assert re.search(r"^# CRASH_CACHE_BIG\b", jl, re.M)
