"""qpn_nodes_set_warm is declared in the header, bound by ctypes, exported by the built library and named by the Julia shim; it
came without a new option, a new flag bit or a new ABI version."""
import ctypes
import os
import re

from qpn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_entry_point_is_declared_bound_and_exported():
    header = _read("include", "qpn_hip.h")
    assert re.search(r"^int qpn_nodes_set_warm\(qpn_ctx \*ctx, qpn_nodes \*nodes, int32_t on\);", header, flags=re.M)
    assert "qpn_nodes_set_warm" in _lib.ABI_SYMBOLS
    lib = _lib.load_library()                             # (raises when a symbol of ABI_SYMBOLS is missing)
    assert lib.qpn_nodes_set_warm.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]
    julia = _read("julia", "QPNHip.jl")
    assert re.search(r"^function nodes_set_warm!\(", julia, flags=re.M) and ":qpn_nodes_set_warm" in julia


def test_no_new_option_flag_or_version():
    header = _read("include", "qpn_hip.h")
    opts = dict(re.findall(r"^#define (QPN_OPT_\w+) (\d+)", header, flags=re.M))
    assert sorted(int(v) for v in opts.values()) == list(range(1, 8)), opts
    flags = dict(re.findall(r"^#define (QPN_AVI_FLAG_\w+|QPN_ABI_VERSION) (\d+)", header, flags=re.M))
    assert flags == {"QPN_ABI_VERSION": "1", "QPN_AVI_FLAG_COLD_START": "1", "QPN_AVI_FLAG_WARM_DUALS": "2"}


def test_the_build_list_has_the_unit():
    assert re.search(r"^units=\(.*\bqpn_warm_mid\b", _read("quadraticprogramnetworks.jl_amd", "csrc", "build.sh"), flags=re.M)
    src = _read("quadraticprogramnetworks.jl_amd", "csrc", "qpn_warm_mid.hip")
    assert "warm_mid_fits(n, k)" in src
