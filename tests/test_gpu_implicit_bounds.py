"""qpn_implicit_bounds (csrc/qpn_lp.hip) against its numpy twin polyhedra.implicit_bounds_host, bit for bit on every output, in every
kernel class and both memory modes; its argument errors and edge cases; and the host functions that use it --
implicit_bounds_batch(route="polyhedron") against the route of the jobs, solve() with the convexity check end to end."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import implicit_cases
from implicit_cases import BY_EXTREMES, BY_POINTS, EMPTY, EXPLICIT, IMPLICIT, ITER_LIMIT, OK, PINNED, UNBOUNDED

pytestmark = pytest.mark.gpu


def _both_modes(engine, A, l, u, **kw):
    """The kernel in host and in device mode against the twin.  -> the twin's answer."""
    import torch
    from qpn_amd import polyhedra
    from qpn_amd.engine import colmajor
    host = (colmajor(A), l, u)
    want = polyhedra.implicit_bounds_host(*host, **kw)
    implicit_cases.same_bits(engine.implicit_bounds(*host, **kw), want, "host mode")
    dv = f"cuda:{engine.device}"
    got = engine.implicit_bounds(*(torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dv) for a in host), **kw)
    assert all(hasattr(v, "cpu") for v in got.values())
    implicit_cases.same_bits(got, want, "device mode")
    return want


@pytest.mark.parametrize("shape", [(1, 1), (3, 2), (8, 4), (16, 8)])
def test_the_family_equals_the_twin_bit_for_bit(engine, shape):
    """50 polyhedra: the last workgroup of the wavefront class holds two of its four."""
    n0 = engine.calls["qpn_implicit_bounds"]
    batch = implicit_cases.family_batch(shape, range(50))
    assert engine.lp_kernel_class(*shape) == 0
    want = _both_modes(engine, *batch)
    assert engine.calls["qpn_implicit_bounds"] == n0 + 2
    every = _both_modes(engine, *batch, all_extremes=True)
    cut = _both_modes(engine, *batch, opts=dict(max_iters=1))
    assert BY_POINTS not in every["how"] and np.all(every["lps"] >= want["lps"])
    if shape == (16, 8):
        seen = set(want["how"].ravel().tolist())
        assert seen & {EXPLICIT, IMPLICIT} and {BY_POINTS, BY_EXTREMES, UNBOUNDED} <= seen
        assert EMPTY in want["status"] and OK in want["status"]
        assert ITER_LIMIT in cut["status"] and (cut["fail_row"] >= 0).any()
        assert want["iters"].max() > 3 and every["lps"].max() == 33


def _class_shapes(engine):
    """(the largest wave-class r, the smallest workgroup-class r, the smallest workspace-class r) at d = 24, 24, 128."""
    r0 = max(r for r in range(1, 200) if engine.lp_kernel_class(r, 24) == 0)
    r2 = min(r for r in range(1, 1025) if engine.lp_kernel_class(r, 128) == 2)
    return (r0, 24), (r0 + 1, 24), (r2, 128)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_class_boundaries_equal_the_twin_bit_for_bit(engine, which):
    r, d = _class_shapes(engine)[which]
    assert engine.lp_kernel_class(r, d) == which and (which == 0 or engine.lp_kernel_class(r - 1, d) == which - 1)
    A, l, u = implicit_cases.boundary_batch(17 + which, r, d)
    want = _both_modes(engine, A, l, u, tol=1e-6)
    assert np.all(want["status"] == OK)
    assert np.all(want["how"][:, 0] == UNBOUNDED) and np.all(want["lo"][:, 0] == -np.inf)          # the row open below
    assert np.all(want["how"][:, 1:3] == IMPLICIT) and np.all(want["eq"][:, 1:3] == 1) and want["eq"].sum() == 6
    assert np.all(want["lps"] < 2 * r) and (which == 2 or np.all(want["lps"] < r)) and want["iters"].max() > 3
    if which == 0:                                                                       # every extreme, where that takes a second or so
        every = _both_modes(engine, A, l, u, tol=1e-6, all_extremes=True)
        assert np.all(every["lps"] == 1 + 2 * r) and np.array_equal(every["eq"], want["eq"])


def test_argument_errors_and_edge_cases(engine):
    from qpn_amd import polyhedra
    from qpn_amd._lib import MEM_HOST
    from qpn_amd.engine import QpnError, colmajor
    # sizes beyond the limits
    for r, d in ((1025, 2), (2, 257)):
        with pytest.raises(QpnError, match="size"):
            engine.implicit_bounds(np.zeros((1, d, r)), np.zeros((1, r)), np.ones((1, r)))
    # inconsistent shapes
    A, l, u = implicit_cases.family_batch((3, 2), range(4))
    for bad in ((colmajor(A), l[:3], u), (colmajor(A), l, u[:, :2]), (colmajor(A)[0], l, u)):
        with pytest.raises(QpnError, match="inconsistent shapes"):
            engine.implicit_bounds(*bad)
    # no polyhedron
    got = engine.implicit_bounds(np.zeros((0, 2, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
    assert got["status"].shape == (0,) and got["eq"].shape == (0, 3)
    # the optional outputs left out: the others are those of the full call
    want = polyhedra.implicit_bounds_host(colmajor(A), l, u)
    Ac = np.ascontiguousarray(colmajor(A)); status = np.full(4, -7, np.int32); eq = np.full((4, 3), 9, np.uint8); vals = np.zeros((4, 3))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = engine.lib.qpn_implicit_bounds(engine.ctx, 4, 3, 2, p(Ac), p(l), p(u), 1e-4, 0, None, p(status), None, p(eq), p(vals), None, None, None,
                                        None, None, MEM_HOST)
    assert rc == 0
    assert np.array_equal(status, want["status"]) and np.array_equal(eq, want["eq"]) and vals.tobytes() == want["vals"].tobytes()
    # a required output missing, an unknown flag
    assert engine.lib.qpn_implicit_bounds(engine.ctx, 4, 3, 2, p(Ac), p(l), p(u), 1e-4, 0, None, p(status), None, None, p(vals), None, None, None,
                                          None, None, MEM_HOST) != 0
    assert engine.lib.qpn_implicit_bounds(engine.ctx, 4, 3, 2, p(Ac), p(l), p(u), 1e-4, 2, None, p(status), None, p(eq), p(vals), None, None, None,
                                          None, None, MEM_HOST) != 0
    # crossed bounds, an all-zero row outside its bounds, an all-explicit polyhedron
    A = np.array([[[1.0, 0.0], [0.0, 1.0]], [[0.0, 0.0], [0.0, 1.0]], [[1.0, 0.0], [0.0, 1.0]]])
    l = np.array([[1.0, 0.0], [1.0, 0.0], [1.0, 2.0]]); u = np.array([[0.0, 1.0], [2.0, 1.0], [1.0, 2.0]])
    want = _both_modes(engine, A, l, u)
    assert want["status"].tolist() == [EMPTY, EMPTY, OK] and want["lps"].tolist() == [0, 1, 1] and want["eq"][2].tolist() == [1, 1]


# ---- the host functions on the polyhedron route against the route of the jobs ---------------------------------------------------
def _random_polys(seed, count, dmax=6, mmax=10):
    """(tests/test_gpu_lp.py's generator, stated again)"""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(count):
        d = int(rng.integers(1, dmax + 1)); m = int(rng.integers(1, mmax + 1))
        A = rng.standard_normal((m, d))
        x0 = rng.standard_normal(d)
        c = A @ x0
        l = c - np.abs(rng.standard_normal(m)) - 0.05; u = c + np.abs(rng.standard_normal(m)) + 0.05
        l = np.where(rng.random(m) < 0.3, -np.inf, l); u = np.where(rng.random(m) < 0.3, np.inf, u)
        if t % 3 == 1 and m >= 2:                      # contradictory pair: a'x <= -1 and a'x >= +1
            A[1] = A[0]; l[0], u[0] = -np.inf, c[0] - 1.0; l[1], u[1] = c[0] + 1.0, np.inf
        if t % 3 == 2 and m >= 2:                      # an equality row
            u[0] = l[0] = c[0]
        out.append((A, l, u))
    return out


def _node_solves(engine):
    return sum(v for k, v in engine.calls.items() if k.startswith("qpn_solve_nodes") or k == "qpn_solve_avi_batch")


def test_implicit_bounds_batch_on_the_polyhedron_route(engine):
    from qpn_amd import polyhedra
    polys = _random_polys(11, 40, dmax=5, mmax=8)
    everything = list(polys)
    polys = [p for p, e in zip(polys, polyhedra.isempty_batch(polys, engine)) if not e]
    polys.append(PINNED)
    assert 20 <= len(polys) < len(everything)
    n0, p0, s0 = engine.calls["qpn_implicit_bounds"], engine.calls["qpn_solve_lps"], _node_solves(engine)
    got = polyhedra.implicit_bounds_batch(polys, engine, route="polyhedron")
    assert engine.calls["qpn_implicit_bounds"] - n0 == len({A.shape for A, _, _ in polys})        # one call per shape
    assert engine.calls["qpn_solve_lps"] == p0 and _node_solves(engine) == s0                     # no LP job, no node solve
    want = polyhedra.implicit_bounds_batch(polys, engine, route="jobs")
    assert engine.calls["qpn_solve_lps"] > p0 and _node_solves(engine) > s0
    for (eq, vals), (eq0, vals0) in zip(got, want):
        assert np.array_equal(eq, eq0)
        assert np.all(np.abs(vals[eq] - vals0[eq]) <= 1e-7)
    assert list(got[-1][0]) == [True, True, True] and np.allclose(got[-1][1], [1.0, 1.0, 0.0], atol=1e-9)
    assert any(eq.any() for eq, _ in got[:-1])
    # the empty set raises, naming the lowest-numbered empty polyhedron of the list
    first = next(k for k, p in enumerate(everything) if not any(p is q for q in polys))
    with pytest.raises(RuntimeError, match=rf"Empty set \(polyhedron {first}\)"):
        polyhedra.implicit_bounds_batch(everything, engine, route="polyhedron")
    with pytest.raises(RuntimeError, match=r"Empty set \(polyhedron 0\)"):
        polyhedra.implicit_bounds_batch([(np.array([[1.0]]), np.array([1.0]), np.array([0.0]))], engine, route="polyhedron")


def test_solve_end_to_end_on_the_polyhedron_route(engine):
    from qpn_amd import algorithm, examples, qp_processing
    off = algorithm.solve(examples.setup("synthetic_pairs", pairs=20, n=8, m=8), engine=engine)
    n0, p0 = engine.calls["qpn_implicit_bounds"], engine.calls["qpn_solve_lps"]
    assert qp_processing.IMPLICIT_BOUNDS_ROUTE == "jobs"
    qp_processing.IMPLICIT_BOUNDS_ROUTE = "polyhedron"
    try:
        on = algorithm.solve(examples.setup("synthetic_pairs", pairs=20, n=8, m=8, check_convexity=True), engine=engine)
    finally:
        qp_processing.IMPLICIT_BOUNDS_ROUTE = "jobs"
    assert engine.calls["qpn_implicit_bounds"] > n0 and engine.calls["qpn_solve_lps"] == p0
    assert on["solved"] and off["solved"]
    assert on["x_opt"].tobytes() == off["x_opt"].tobytes()
