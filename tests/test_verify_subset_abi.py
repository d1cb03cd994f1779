"""The ABI of the subset verify (qpn_verify_nodes_subset_h), checked without a GPU: the header's declaration, the
symbol table of the Python binding, the built library's export and its answer to a null context, and Nodes.verify_subset."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["qpn_ctx *ctx", "qpn_nodes *nodes", "int32_t count", "const int32_t *idx", "const double *xd", "const double *w",
        "int64_t stride_w", "double tol", "int32_t *solution", "double *lambda", "int32_t *path", "int mem"]


def _header():
    return open(os.path.join(ROOT, "include", "qpn_hip.h")).read()


def test_header_declares_the_entry_point():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decl = re.search(r"int\s+qpn_verify_nodes_subset_h\s*\(([^;]*)\)\s*;", src)
    assert decl, "include/qpn_hip.h does not declare qpn_verify_nodes_subset_h"
    assert [" ".join(a.split()) for a in decl.group(1).split(",")] == ARGS


def test_header_documents_path_6():
    doc = re.search(r"path \[batch\] int32: 0 infeasible.*?\*/", _header(), flags=re.S)
    assert doc and re.search(r"\b6 no such node", doc.group(0)), "path 6 is not documented next to the other path codes"


def test_binding_names_and_library_exports_it():
    import qpn_amd  # noqa: F401
    from qpn_amd import _lib
    assert "qpn_verify_nodes_subset_h" in _lib.ABI_SYMBOLS
    lib = _lib.load_library()                    # raises if the library lacks any symbol of ABI_SYMBOLS
    fn = lib.qpn_verify_nodes_subset_h
    assert len(fn.argtypes) == len(ARGS)
    # a null context is refused before anything else is looked at
    raw = ctypes.CDLL(_lib.LIB_PATH).qpn_verify_nodes_subset_h
    raw.restype = ctypes.c_int
    assert raw(None, None, 0, None, None, None, ctypes.c_int64(0), ctypes.c_double(1e-4), None, None, None, 0) == -1   # QPN_ERR_ARG


def test_nodes_has_verify_subset():
    import inspect

    import qpn_amd  # noqa: F401
    from qpn_amd import engine
    assert list(inspect.signature(engine.Nodes.verify_subset).parameters) == ["self", "idx", "xd", "w", "tol"]
