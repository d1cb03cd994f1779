"""QPN_AVI_FLAG_WARM_DUALS is one value in the header, the ctypes binding and the Julia shim, beside QPN_AVI_FLAG_COLD_START, and
the ABI version did not move."""
import os
import re

from qpn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_flag_has_one_value_everywhere():
    header = _read("include", "qpn_hip.h")
    defs = dict(re.findall(r"^#define (QPN_AVI_FLAG_\w+|QPN_ABI_VERSION) (\d+)", header, flags=re.M))
    assert defs == {"QPN_ABI_VERSION": "1", "QPN_AVI_FLAG_COLD_START": "1", "QPN_AVI_FLAG_WARM_DUALS": "2"}
    assert (_lib.AVI_FLAG_COLD_START, _lib.AVI_FLAG_WARM_DUALS) == (1, 2)
    julia = _read("julia", "QPNHip.jl")
    assert re.search(r"^const QPN_AVI_FLAG_WARM_DUALS = Int32\(2\)", julia, flags=re.M)
    assert "warm::Union{Nothing,Matrix{Float64}} = nothing" in julia


def test_the_build_list_has_the_unit():
    assert re.search(r"^units=\(.*\bqpn_warm\b", _read("quadraticprogramnetworks.jl_amd", "csrc", "build.sh"), flags=re.M)
    assert os.path.exists(os.path.join(ROOT, "quadraticprogramnetworks.jl_amd", "csrc", "qpn_warm.hip"))
