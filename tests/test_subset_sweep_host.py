"""The host side of the subset sweep (qpn_solve_nodes_subset_h): the route switch of solve_level and the ABI.

Route: a stand-in engine, the CPU oracle behind a resident handle that has solve and solve_subset; both solve the rows they are
asked for and count them.  With level_batch.SUBSET_SWEEP_ROUTE on, a solve_level sweep with a `settled` set hands over exactly the
records of the unsettled leaf players and x_opt equals the route being off, bit for bit; with it off every record of the level's
batch is solved.  ABI: the header declares the entry point and the built library exports it."""
import ctypes
import os
import re

import numpy as np

from oracle_engine import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _CountingHandle:
    """Nodes.solve and Nodes.solve_subset on host arrays, served by the oracle's solve_nodes over the rows asked for."""

    def __init__(self, eng, records):
        self.eng, self.records = eng, [np.array(a) for a in records]
        self.batch, self.n = self.records[2].shape
        self.m = self.records[5].shape[1]

    def _rows(self, rows, w):
        self.eng.solved += len(rows)
        res = OracleEngine.solve_nodes(self.eng, *[a[rows] for a in self.records], w)
        return {k: np.array(res[k]) for k in ("z", "status", "resid", "pivots")}

    def solve(self, w, opts=None, want=("z", "resid", "pivots", "active"), out=None, x_out=None, warm=None):
        assert warm is None and np.shape(w)[0] == self.batch
        self.eng.full_calls += 1
        return self._rows(np.arange(self.batch), w)

    def solve_subset(self, idx, w, opts=None, want=("z", "resid", "pivots", "active"), out=None, x_out=None, warm=None):
        idx = np.asarray(idx)
        assert warm is None and idx.dtype == np.int32 and idx.ndim == 1 and np.shape(w) == (idx.size, self.records[1].shape[1])
        assert idx.size == np.unique(idx).size and idx.min() >= 0 and idx.max() < self.batch
        self.eng.subset_calls.append(idx.copy())
        return self._rows(idx, w)


class _CountingEngine(OracleEngine):
    def __init__(self):
        super().__init__()
        self.solved, self.full_calls, self.subset_calls = 0, 0, []

    def upload_nodes(self, *records):
        return _CountingHandle(self, records)


def _net():
    from qpn_amd import examples
    net = examples.setup("synthetic_pairs", pairs=6, n=3, m=4)
    followers = sorted(i for i in net.qps if not net.network_edges[i])
    x = 0.1 * np.random.default_rng(5).standard_normal(net.num_vars)
    return net, followers, x


def _sweep(route, settled):
    from qpn_amd import level_batch
    net, followers, x = _net()
    eng = _CountingEngine()
    assert level_batch.SUBSET_SWEEP_ROUTE is False
    level_batch.SUBSET_SWEEP_ROUTE = route
    try:
        x_opt = level_batch.solve_level(net, followers, x, engine=eng, settled=settled(followers))
    finally:
        level_batch.SUBSET_SWEEP_ROUTE = False
    return x_opt, eng, followers, x


def test_route_solves_exactly_the_unsettled_leaf_records():
    settled = lambda f: set(f[1::2]) | {f[0]}                       # 4 of 6 settled, 2 left, not adjacent
    off, e0, followers, x = _sweep(False, settled)
    on, e1, _, _ = _sweep(True, settled)
    left = [i for i in followers if i not in settled(followers)]
    assert len(left) == 2
    # off: the code as it was -- every record of the level's batch, one full call
    assert e0.solved == len(followers) and e0.full_calls == 1 and not e0.subset_calls
    # on: the unsettled players' records and nothing else
    assert e1.solved == len(left) and e1.full_calls == 0 and len(e1.subset_calls) == 1
    assert np.array_equal(on, off)
    assert not np.array_equal(on, x)                                # (the sweep moved something)
    from qpn_amd import level_batch
    moved = np.flatnonzero(on != x)
    owned = set(np.concatenate([np.asarray(level_batch.node_record(_net()[0], i)["dec"]) for i in left]).tolist())
    assert set(moved.tolist()) <= owned


def test_route_is_not_taken_without_a_record_to_leave_out():
    off, e0, followers, _ = _sweep(False, lambda f: set())
    on, e1, _, _ = _sweep(True, lambda f: set())
    assert e1.full_calls == 1 and not e1.subset_calls and e1.solved == len(followers) == e0.solved
    assert np.array_equal(on, off)


def test_route_yields_to_the_warm_route():
    from qpn_amd import level_batch
    net, followers, x = _net()

    class _Warm(_CountingHandle):
        def solve(self, w, opts=None, want=(), out=None, x_out=None, warm=None):
            self.eng.full_calls += 1
            return self._rows(np.arange(self.batch), w)

    class _WarmEngine(_CountingEngine):
        def upload_nodes(self, *records):
            return _Warm(self, records)

    eng = _WarmEngine()
    level_batch.SUBSET_SWEEP_ROUTE = True
    level_batch.WARM_DUALS_ROUTE = True
    try:
        level_batch.solve_level(net, followers, x, engine=eng, settled={followers[0]})
    finally:
        level_batch.SUBSET_SWEEP_ROUTE = False
        level_batch.WARM_DUALS_ROUTE = False
    assert eng.full_calls == 1 and not eng.subset_calls


def test_header_declares_and_library_exports_the_entry_point():
    import qpn_amd  # noqa: F401
    from qpn_amd import _lib
    src = open(os.path.join(ROOT, "include", "qpn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = re.search(r"int\s+qpn_solve_nodes_subset_h\s*\(([^;]*)\)\s*;", src)
    assert decl, "include/qpn_hip.h does not declare qpn_solve_nodes_subset_h"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == 15 and args[2] == "int32_t count" and args[3] == "const int32_t *idx"
    assert "qpn_solve_nodes_subset_h" in _lib.ABI_SYMBOLS
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "qpn_solve_nodes_subset_h")
    # a null context is refused before anything else is looked at
    lib.qpn_solve_nodes_subset_h.restype = ctypes.c_int
    assert lib.qpn_solve_nodes_subset_h(*([None] * 2), 0, *([None] * 2), ctypes.c_int64(0), *([None] * 6), 0, None,
                                        ctypes.c_int64(0)) == -1
